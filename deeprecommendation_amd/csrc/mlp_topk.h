// Fused MLP score-and-select (ncf_mlp_topk): the k best items of each listed user for an MLP readout (BasicNCF: cat(user, item);
// GraphNCF(use_dot_product=False): cat(item, user)), without the B x I pair id columns or score matrix.
//
// Scores: bit-identical to score_fused_f32_kernel (mlp_fused.hip) for the same pair and packed blob.  That kernel computes every
// layer transposed (pair on the MFMA column, neuron on the accumulator rows, v_mfma_f32_32x32x2_f32), starts layer 1's accumulator
// at b1 and runs the k-steps of the concat's first part (q < EA/8, rows of tabA) before those of the second part.  An MFMA column
// depends only on its own B operands, so after step EA/8 - 1 the accumulator of a pair is a function of its first-part row alone:
//   prefix pass   mlp_prefix_kernel runs exactly those first EA/8 k-steps (same Wp1 fragments, same j order, from b1) once per
//                 first-part row (32 rows per wave tile) and writes the N1-float state in neuron order: per listed user in the
//                 user-first order, per ranked column in the item-first order.
//   main kernel   one wave = one user x a range of ranked columns, 32 columns (one MFMA tile) at a time.  Layer 1's accumulator
//                 starts from the prefix state (user-first: the user's state, broadcast over the columns and loaded like b1;
//                 item-first: each column's own state), the remaining Q1 - EA/8 k-steps take the second part's rows (item rows
//                 per column, or the user row broadcast), then layer 2 and the 1-wide layer are the fused kernel's own code
//                 (fused_layer2, fused_last_sum: mlp_fused.h).  The same operations run on the same operands in the same order,
//                 so every score has the fused scorer's bits; the first part's FLOP (2 EA N1 per pair) is paid once per row
//                 instead of once per pair.
// Selection: per wave, the user's candidate keys (map(score) << 32 | ~column, the topk.hip order) live in LDS behind a running k-th
// key threshold; excluded columns are skipped through an LDS bitmap of the range.  A buffer that cannot take another 32 keys is
// re-selected down to k (wave_reselect).  Each (user, range) writes its k best keys in the layout topk_tile_kernel's merge levels
// read (kp keys per range, 0-padded), and those levels (topk_merge, topk.hip) finish the ranking; the last one recovers each score
// from its key (topk_unmap).
// A fused-MLP score is never -0.0: `partial` starts at +0.f, an fmaf onto +0 and an exact cancellation both give +0 in
// round-to-nearest, so partial is never -0 and partial + bl is -0 only if both are.  The recovered bits are therefore the caller's
// for every non-NaN score; NaN payloads are not kept (a NaN ranks last and comes back as a NaN).
// Host side: ncf_mlp_topk and ncf_mlp_rank (the same waves with a counting sink, rank_common.h) share one front end: the operand
// refusals (mlp_check_operands), the prefix launch with the scoring part of the kernel arguments (mlp_prefix_pass) and the column
// ranges (mlp_tile_cols).  Each keeps what differs: the merge plan and chunk loop, or the target preparation and the sink's fields.
//
// This header holds the kernels and the two entry points' bodies (mlp_topk_run, mlp_rank_run) because two files instantiate them:
// mlp_topk.hip for the MLP readout (ncf_mlp_topk, ncf_mlp_rank) and neumf.hip for NeuMF (ncf_neumf_topk, ncf_neumf_rank), whose
// score is the same wave's s_mlp plus a GMF term g added before the sink (gmf.h has the term and its contract).  The switch is the
// argument type: Args::kGmf.  With it off no GMF code exists and the instantiations are the ones this kernel had before it was
// shared (same mangled names, registers, scratch, LDS and instructions: DESIGN 4.41 has the tables).  Internal: not part of the ABI.
#pragma once
#include <type_traits>

#include "gmf.h"
#include "mlp_fused.h"
#include "rank_common.h"
#include "topk_common.h"

namespace ncf {

constexpr int kMtWaves = 4;                      // waves per workgroup (independent: no workgroup barrier)
constexpr int kMtThreads = kMtWaves * kWave;
constexpr int kMtCols = 32;                      // columns per wave tile (the MFMA N dimension)
constexpr int kMtCap = 256;                      // candidate keys per wave (= wave_kth's 4 x 64)
constexpr int kMtMaxK = 128;                     // fused limit on k (a re-select must free >= 32 + some slots)
constexpr int64_t kMtTargetWaves = 2048;         // range shrinks (8192 -> 32 columns) until the grid has this many waves

// State of layer 1 after the first part's k-steps for n first-part rows tab[idx[p]] (tab[p] with idx NULL):
// state[p][n] = (b1 + W1[:, :EA] . row)[n], accumulated in score_fused_f32_kernel's order.  Out-of-range ids read row 0 scaled
// by zero (as the fused kernel does) and set the flag.  (layer1_partial_kernel, mlp_partial.hip, is this computation with a
// look-ahead; see there why both exist.)
template <int K0, int N1>
__global__ __launch_bounds__(256) void mlp_prefix_kernel(const float* __restrict__ tab, int64_t rows, int64_t ld,
                                                         const int64_t* __restrict__ idx, int64_t n, int EA,
                                                         const float* __restrict__ Wp1, const float* __restrict__ b1,
                                                         float* __restrict__ state, int32_t* oob) {
    constexpr int NT1 = N1 / 32;
    const int lane = threadIdx.x & 63;
    const int m = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 32 >= n) return;
    const int64_t p = tile * 32 + m;
    const int64_t pc = p < n ? p : n - 1;
    const int64_t ia = idx ? idx[pc] : pc;
    const bool ok = (ia >= 0) & (ia < rows);
    if (!ok && oob) *oob = 1;
    const float* row = tab + (ok ? ia : 0) * ld + 4 * h;
    const float z = ok ? 1.f : 0.f;
    f32x16 acc[NT1];
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) fused_load_tile(acc[nt], b1, nt, h);
    const f32x4* wp = reinterpret_cast<const f32x4*>(Wp1) + lane;
    const int qa = EA / 8;
    for (int q = 0; q < qa; ++q) {
        const f32x4 xb = fused_ldg4(row + 8 * q) * z;
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) {
            const f32x4 w = wp[(q * NT1 + nt) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], xb[j], acc[nt], 0, 0, 0);
        }
    }
    if (p >= n) return;
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) fused_store_tile(state + p * N1, acc[nt], nt, h);
}

struct MtArgs {
    static constexpr bool kGmf = false;               // no GMF term: the MLP readout (GmfArgs turns it on)
    const float* tabB; int64_t rowsB; int64_t ldB;   // the concat's second part (items user-first, users item-first)
    const int64_t* idxU; const int64_t* idxI;         // user ids (read here item-first only), item ids (read here user-first only)
    int user_first;
    int64_t cols; int EA;
    const float* state;                               // prefix state: per global row (user-first) or per column (item-first)
    const float* Wp1; const float* Wp2; const float* b2; const float* wl; const float* bl;
    const int64_t* seen_rowptr; const int32_t* seen_col;
    int64_t row0, nrows; int tiles, tile_cols, k, kp;
    unsigned long long* out_keys; int64_t n_out;
    int32_t* oob;
};

struct MtWaveShared {
    unsigned long long buf[kMtCap];
    uint32_t bitmap[kTopkTile / 32];
};

// ncf_mlp_rank: the same waves with a counting sink (rank_common.h) instead of the candidate buffer
struct MrArgs : MtArgs {
    const int64_t* tgt_rowptr; const unsigned long long* skey; const int32_t* sperm;   // the rows' sorted target keys and places
    int max_targets, P;                               // targets ranked per row; its LDS slots (a power of two)
    int32_t* rank; int32_t* ranked;
};

// the rank sinks' LDS per wave: the range's exclusion bitmap; ONE (a single target: key and counter in registers) nothing else,
// else the row's sorted target keys and the histogram over them.  2.6 KB per wave at most, so it is static.
template <bool ONE>
struct MrWaveShared {
    uint32_t bitmap[kTopkTile / 32];
    unsigned long long buf[ONE ? 1 : kRankMaxTargets];
    uint32_t hist[ONE ? 1 : kRankMaxTargets + 1];
};

enum { kMtSinkTopk = 0, kMtSinkRankOne = 1, kMtSinkRank = 2 };
template <int SINK> struct MtSinkShared { typedef MrWaveShared<SINK == kMtSinkRankOne> type; };
template <> struct MtSinkShared<kMtSinkTopk> { typedef MtWaveShared type; };

// NeuMF (user-first only): the arguments and the wave's LDS of either sink, plus the GMF term's.  trow: the rounded w (.) p_u row of
// every listed user (D floats per row of the result, written by gmf_trow_kernel); a wave keeps its user's in LDS, not in VGPRs.
template <class Base>
struct GmfArgs : Base {
    static constexpr bool kGmf = true;
    const float* tabQ; int64_t ldQ;                   // the items' GMF table: the rows of tabB's ids (rowsB rows)
    const float* trow; int D;
};
template <class Base>
struct GmfShared : Base {
    __attribute__((aligned(16))) float t[kGmfMaxD];
};

// SINK says what a wave does with a score: the top-K candidate buffer behind a threshold (Args = MtArgs), a register counter
// against the row's one target key, or a binary search into the row's sorted target keys and a bump of the histogram (MrArgs).
template <int K0, int N1, int N2, int SINK, class Args>
__global__ __launch_bounds__(kMtThreads, 2) void mlp_topk_kernel(Args a) {
    constexpr int NT1 = N1 / 32, Q1 = K0 / 8;
    constexpr int NT2 = N2 / 32;
    constexpr bool GMF = Args::kGmf;
    // chunks of a column's GMF row requested before layer 1 (4: all of it up to D = 32); the 256-128 tower has no register to spare
    constexpr int kGmfAhead = (N1 >= 256 && N2 >= 128) ? 0 : 4;
    typedef typename MtSinkShared<SINK>::type SinkShared;
    typedef std::conditional_t<GMF, GmfShared<SinkShared>, SinkShared> Shared;
    __shared__ Shared shw[kMtWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Shared& sh = shw[wave];
    const int m = lane & 31, h = lane >> 5;
    const int64_t unit = (int64_t)blockIdx.x * kMtWaves + wave;
    if (unit >= a.nrows * a.tiles) return;               // whole wave exits together
    const int64_t uloc = unit / a.tiles, r = a.row0 + uloc;
    const int range = (int)(unit % a.tiles);
    const int64_t c0 = (int64_t)range * a.tile_cols, c1 = min(a.cols, c0 + a.tile_cols);
    const bool excl = a.seen_rowptr != nullptr;
    if (excl) {                                          // the user's excluded columns inside [c0, c1)
        for (int w = lane; w < a.tile_cols / 32; w += kWave) sh.bitmap[w] = 0u;
        wave_lds_sync();
        const int64_t pb = a.seen_rowptr[r], pe = a.seen_rowptr[r + 1];
        for (int64_t p = pb + lane; p < pe; p += kWave) {
            const int64_t c = (int64_t)a.seen_col[p] - c0;   // duplicates and ids outside the range do nothing
            if (c >= 0 && c < c1 - c0) atomicOr(&sh.bitmap[c >> 5], 1u << (c & 31));
        }
        wave_lds_sync();
    }
    // item-first: the user is the second part, one row broadcast to every column
    const float* urow = nullptr;
    float zU = 1.f;
    if (!a.user_first) {
        const int64_t iu = a.idxU ? a.idxU[r] : r;
        const bool ok = (iu >= 0) & (iu < a.rowsB);
        if (!ok && a.oob) *a.oob = 1;
        urow = a.tabB + (ok ? iu : 0) * a.ldB + 4 * h;
        zU = ok ? 1.f : 0.f;
    }
    const int qa = a.EA / 8, Qr = Q1 - qa;               // k-steps done by the prefix pass / left here (Qr >= 1)
    const float bl0 = a.bl[0];
    unsigned long long thr = 0ull;
    int cnt = 0;
    // keep the wave's k best candidates; returns the k-th key (the new threshold)
    auto reselect = [&]() {
        wave_lds_sync();
        const unsigned long long kth = wave_reselect(sh.buf, cnt, a.k, lane);
        wave_lds_sync();
        cnt = a.k;
        return kth;
    };
    [[maybe_unused]] int64_t tb = 0;                     // rank sinks: the row's first target entry and its chunk length
    [[maybe_unused]] int tn = 0;
    if constexpr (SINK != kMtSinkTopk) {
        tb = a.tgt_rowptr[r];
        tn = (int)min((int64_t)a.max_targets, a.tgt_rowptr[r + 1] - tb);
        if constexpr (SINK == kMtSinkRankOne) {
            thr = tn > 0 ? a.skey[tb] : kRankNoKey;     // the target's key: a column counts when its key is greater
        } else {
            rank_stage(sh.buf, sh.hist, a.skey + tb, tn, a.P, lane, kWave);
            wave_lds_sync();
        }
        int ex = 0;                                     // ranked: the range's columns minus the excluded ones
        if (excl)
            for (int w = lane; w < a.tile_cols / 32; w += kWave) ex += __popc(sh.bitmap[w]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ex += __shfl_xor(ex, o);
        if (lane == 0) atomicAdd(&a.ranked[r], (int)(c1 - c0) - ex);
    }
    if constexpr (GMF) {                                 // the user's t row: every tile reads it chunk by chunk (gmf.h)
        for (int d = lane; d < a.D; d += kWave) sh.t[d] = a.trow[r * a.D + d];
        wave_lds_sync();
    }

    for (int64_t cb = c0; cb < c1; cb += kMtCols) {
        // The bias / weight pointers are made opaque per tile: hoisted out of the tile loop, the loop-invariant b2, wl and first
        // weight loads would hold ~160 VGPRs for the whole loop and spill.
        const float* Wp1 = a.Wp1;
        const float* Wp2 = a.Wp2;
        const float* b2 = a.b2;
        const float* wl = a.wl;
        asm volatile("" : "+s"(Wp1), "+s"(Wp2), "+s"(b2), "+s"(wl));
        const int64_t c = cb + m;
        const int64_t cc = c < c1 ? c : c1 - 1;
        const float* srow;
        const float* xrow;
        float zx;
        [[maybe_unused]] const float* qrow = nullptr;    // GMF: the column's row of the items' GMF table, and whether its id is in range
        [[maybe_unused]] bool okq = false;
        if (a.user_first) {
            srow = a.state + r * N1;
            const int64_t ib = a.idxI ? a.idxI[cc] : cc;
            const bool ok = (ib >= 0) & (ib < a.rowsB);
            if (!ok && a.oob) *a.oob = 1;
            xrow = a.tabB + (ok ? ib : 0) * a.ldB + 4 * h;
            zx = ok ? 1.f : 0.f;
            if constexpr (GMF && kGmfAhead > 0) {
                qrow = a.tabQ + (ok ? ib : 0) * a.ldQ + 4 * h;
                okq = ok;
            }
        } else {
            srow = a.state + cc * N1;
            xrow = urow;
            zx = zU;
        }

        // ---- layer 1: acc1 = prefix state + the second part's k-steps (score_fused_f32_kernel's steps qa .. Q1 - 1) ----
        f32x16 acc1[NT1];
        [[maybe_unused]] f32x4 qpre[GMF && kGmfAhead ? kGmfAhead : 1];   // GMF: the first chunks of qrow, in flight under layers 1 and 2
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) fused_load_tile(acc1[nt], srow, nt, h);
        {
            // Qr is a runtime count, so the steps run in a loop of step pairs with two weight buffers (a fully unrolled loop with
            // per-step guards keeps both versions of every ring register live and spills).  As in the fused kernel, the next
            // step's weight load for tile nt is issued right behind tile nt's MFMAs, and the row chunks two and three steps ahead
            // are issued after the step's weight loads, so the in-order vmcnt wait for the next weights never waits for them.
            // Look-ahead loads past the last step re-read the last step's data (in bounds, unused) instead of branching.
            const f32x4* wp = reinterpret_cast<const f32x4*>(Wp1) + (int64_t)qa * NT1 * 64 + lane;  // + (s*NT1 + nt)*64
            auto mfma_step = [&](const f32x4 (&w)[NT1], f32x4 (&wn)[NT1], int sn, f32x4 xv) {
                const f32x4 xb = xv * zx;                // zero an out-of-range row at use time
#pragma unroll
                for (int nt = 0; nt < NT1; ++nt) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nt][j], xb[j], acc1[nt], 0, 0, 0);
                    wn[nt] = wp[(sn * NT1 + nt) * 64];
                }
            };
            f32x4 wA[NT1], wB[NT1];
            f32x4 x0, x1, x2, x3;
#pragma unroll
            for (int nt = 0; nt < NT1; ++nt) wA[nt] = wp[nt * 64];
            x0 = fused_ldg4(xrow);
            x1 = fused_ldg4(xrow + 8 * min(1, Qr - 1));
            if constexpr (GMF) {                         // behind the first step's weights and rows: no wait of that step is for these
#pragma unroll
                for (int g = 0; g < kGmfAhead; ++g) qpre[g] = fused_ldg4(qrow + 8 * min(g, a.D / 8 - 1));
            }
            int s = 0;
            for (; s + 1 < Qr; s += 2) {
                mfma_step(wA, wB, s + 1, x0);
                x2 = fused_ldg4(xrow + 8 * min(s + 2, Qr - 1));
                x3 = fused_ldg4(xrow + 8 * min(s + 3, Qr - 1));
#pragma unroll
                for (int nt = 0; nt < NT1; ++nt) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
                }
                __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(wB, wA, min(s + 2, Qr - 1), x1);
#pragma unroll
                for (int nt = 0; nt < NT1; ++nt) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                x0 = x2;
                x1 = x3;
            }
            if (s < Qr) {                                // odd count: the last step (wA, x0 hold it)
                const f32x4 xb = x0 * zx;
#pragma unroll
                for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wA[nt][j], xb[j], acc1[nt], 0, 0, 0);
            }
        }

        // ---- layer 2 and the 1-wide layer: the fused kernel's code (mlp_fused.h); bl[0] was read before the tile loop ----
        float score;
        if constexpr (N2 > 0) {
            f32x16 acc2[NT2];
            fused_layer2<N1, N2>(acc1, acc2, b2, Wp2, lane);
            score = fused_last_sum(acc2, wl, lane);
        } else {
            score = fused_last_sum(acc1, wl, lane);
        }
        // NeuMF: fl(s_mlp + g) before the bias.  g is never -0.0 (gmf.h) and s_mlp is not (above), so neither is their sum, and the
        // score is -0.0 only if the sum and bl both are: topk_unmap still returns the caller's bits for every non-NaN score.
        if constexpr (GMF && kGmfAhead == 0) {           // nothing was requested ahead: the row's address is formed here, not held
            const int64_t ib = a.idxI ? a.idxI[cc] : cc;
            okq = (ib >= 0) & (ib < a.rowsB);
            qrow = a.tabQ + (okq ? ib : 0) * a.ldQ + 4 * h;
        }
        if constexpr (GMF) {
            int toff = 4 * h, nS = a.D;                  // opaque per tile, like the weight pointers above: nothing of the term is
            asm volatile("" : "+v"(toff), "+s"(nS));     // hoisted out of the tile loop into registers the layers need
            score = score + gmf_dot_t<kGmfAhead>(sh.t + toff, qrow, okq, nS / 8, qpre);
        }
        score = score + bl0;

        // ---- select: lanes of half 0 hold columns cb + m ----
        const unsigned long long key = ((unsigned long long)topk_map(score) << 32) | (0xFFFFFFFFu - (uint32_t)c);
        if constexpr (SINK == kMtSinkTopk) {
            bool pass = h == 0 && c < c1 && key > thr;
            if (pass && excl) {
                const int off = (int)(c - c0);
                pass = !((sh.bitmap[off >> 5] >> (off & 31)) & 1u);
            }
            const unsigned long long mk = __ballot(pass);
            if (pass) sh.buf[cnt + lanes_below(mk)] = key;   // cnt <= kMtCap - 32 before this tile
            cnt += __popcll(mk);
            if (cnt > kMtCap - kMtCols) thr = reselect();
        } else {
            bool pass = h == 0 && c < c1;
            if (pass && excl) {
                const int off = (int)(c - c0);
                pass = !((sh.bitmap[off >> 5] >> (off & 31)) & 1u);
            }
            if constexpr (SINK == kMtSinkRankOne) {
                cnt += (pass && key > thr) ? 1 : 0;      // private counter, reduced once after the range
            } else if (pass) {
                const int pos = rank_lower_bound(sh.buf, a.P, key);
                if (pos) atomicAdd(&sh.hist[pos], 1u);
            }
        }
    }

    if constexpr (SINK == kMtSinkTopk) {
        // this range's k best keys, unsorted, 0-padded to kp
        if (cnt > a.k) reselect();
        wave_lds_sync();
        unsigned long long* dst = a.out_keys + uloc * a.n_out + (int64_t)range * a.kp;
        for (int s = lane; s < a.kp; s += kWave) dst[s] = s < cnt ? sh.buf[s] : 0ull;
    } else if constexpr (SINK == kMtSinkRankOne) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0 && cnt && thr != kRankNoKey) atomicAdd(&a.rank[tb], cnt);   // a chunk of one: place 0
    } else {
        wave_lds_sync();
        if (lane == 0) rank_suffix(sh.hist, a.P);
        wave_lds_sync();
        rank_flush(sh.buf, sh.hist, a.sperm + tb, tn, a.rank + tb, lane, kWave);
    }
}

// The main kernel's column ranges: tile_cols shrinks (8192 -> floor_cols) until the grid has kMtTargetWaves waves.  Top-K and the
// one-target rank sink go down to one MFMA tile (kMtCols); a range with target chunks in LDS stays >= kMrChunkCols columns (its
// staging, suffix sum and flush are paid per range).
constexpr int kMrChunkCols = 512;
static int mlp_tile_cols(int64_t rows, int64_t cols, int floor_cols) {
    int tile_cols = kTopkTile;
    while (tile_cols > floor_cols && rows * ((cols + tile_cols - 1) / tile_cols) < kMtTargetWaves) tile_cols >>= 1;
    return tile_cols;
}

// the merge levels after it, over kp keys per range
static TopkMerge mlp_topk_plan(int64_t rows, int64_t cols, int tile_cols, int k) {
    return topk_merge_plan(rows, (cols + tile_cols - 1) / tile_cols * topk_kp(k), k);
}

// the prefix state at the front of the workspace: N1 floats per user (user-first) or per ranked column (item-first)
static size_t mlp_state_bytes(int64_t rows, int64_t cols, int N1, int user_first) {
    return (size_t)(user_first ? rows : cols) * N1 * sizeof(float);
}

// A = MtArgs / MrArgs (mlp_topk.hip) or GmfArgs of either (neumf.hip): a file compiles the instances of the types it launches
template <class A>
static void mt_dispatch(int K0, int N1, int N2, unsigned blocks, hipStream_t s, const A& a) {
#define X(k0, n1, n2) \
    if (K0 == k0 && N1 == n1 && N2 == n2) hipLaunchKernelGGL((mlp_topk_kernel<k0, n1, n2, kMtSinkTopk, A>), dim3(blocks), dim3(kMtThreads), 0, s, a);
    NCF_FUSED_INSTANCES(X)
#undef X
}

template <class A>
static void mr_dispatch(int K0, int N1, int N2, bool one, unsigned blocks, hipStream_t s, const A& a) {
#define X(k0, n1, n2) \
    if (K0 == k0 && N1 == n1 && N2 == n2) { \
        if (one) hipLaunchKernelGGL((mlp_topk_kernel<k0, n1, n2, kMtSinkRankOne, A>), dim3(blocks), dim3(kMtThreads), 0, s, a); \
        else hipLaunchKernelGGL((mlp_topk_kernel<k0, n1, n2, kMtSinkRank, A>), dim3(blocks), dim3(kMtThreads), 0, s, a); \
    }
    NCF_FUSED_INSTANCES(X)
#undef X
}

static bool mt_instance(int K0, int N1, int N2) {
#define X(k0, n1, n2) \
    if (K0 == k0 && N1 == n1 && N2 == n2) return true;
    NCF_FUSED_INSTANCES(X)
#undef X
    return false;
}

static bool mt_shape_ok(int dtype, int EA, int EB, int n_layers, const int* dims) {
    if (dtype != NCF_F32 || !dims) return false;
    if (n_layers != 2 && n_layers != 3) return false;
    if (dims[n_layers] != 1) return false;
    if (EA < 8 || EB < 8 || EA % 8 || EB % 8 || EA + EB != dims[0]) return false;   // both parts present
    return mt_instance(dims[0], dims[1], n_layers == 3 ? dims[2] : 0);
}

static int mt_check(int64_t rows, int64_t cols, int k, const char* what) {
    if (const int rc = topk_check_k(what, k, kMtMaxK)) return rc;
    return topk_check_size(what, rows, cols);
}

static int mr_check(int64_t rows, int64_t cols, int max_targets, const char* what) {
    if (const int rc = rank_check_max_targets(what, max_targets)) return rc;
    return topk_check_size(what, rows, cols);
}

// ncf_mlp_topk's column ranges and merge plan; ncf_mlp_rank's column ranges (one target: the top-K floor)
static TopkMerge mt_plan(int64_t rows, int64_t cols, int k, int* tile_cols) {
    const int tc = mlp_tile_cols(rows, cols, kMtCols);
    if (tile_cols) *tile_cols = tc;
    return mlp_topk_plan(rows, cols, tc, k);
}
static int mr_tile_cols(int64_t rows, int64_t cols, int max_targets) {
    return mlp_tile_cols(rows, cols, max_targets == 1 ? kMtCols : kMrChunkCols);
}

// The refusals both entry points make after their own limit check (mt_check / mr_check), in their order; `what` names the entry
// point.  n_targets: 0 from ncf_mlp_topk; outputs: the caller's output pointers that share the "null argument" refusal are all
// there.  rows == 0 passes before any pointer is looked at: the caller returns NCF_OK then.
static int mlp_check_operands(const char* what, int dtype, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB,
                              int64_t ldB, int EA, int EB, int user_first, const int64_t* user_ids, const int64_t* item_ids, int64_t rows,
                              int64_t cols, int n_layers, const int* dims, const void* packed, int64_t n_targets, bool outputs) {
    if (!mt_shape_ok(dtype, EA, EB, n_layers, dims))
        return fail(NCF_EUNSUPPORTED, "%s: no fused instance for dtype=%d EA=%d EB=%d layers=%d", what, dtype, EA, EB, n_layers);
    if (n_targets < 0) return fail(NCF_EINVAL, "%s: n_targets = %lld", what, (long long)n_targets);
    if (rows == 0) return NCF_OK;
    if (!tabA || !tabB || !packed || !outputs) return fail(NCF_EINVAL, "%s: null argument", what);
    if (ldA < EA || ldB < EB || ldA % 4 || ldB % 4 || !aligned16(tabA) || !aligned16(tabB) || !aligned16(packed))
        return fail(NCF_EINVAL, "%s: tables must be 16-byte aligned with ld %% 4 == 0", what);
    const int64_t nUrows = user_first ? rowsA : rowsB, nIrows = user_first ? rowsB : rowsA;
    if (!user_ids && rows > nUrows) return fail(NCF_EINVAL, "%s: rows = %lld > user table rows without user ids", what, (long long)rows);
    if (!item_ids && cols > nIrows) return fail(NCF_EINVAL, "%s: cols = %lld > item table rows without item ids", what, (long long)cols);
    return NCF_OK;
}

// Launches the prefix pass over the first part's rows (the listed users user-first, the ranked items item-first) into `state` and
// fills the scoring part of the main kernel's arguments.  The column ranges, the rows and the sink's fields are the caller's.
static void mlp_prefix_pass(MtArgs& a, const void* tabA, int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB, int EA,
                            int user_first, const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, int n_layers,
                            const int* dims, const void* packed, const int64_t* seen_rowptr, const int32_t* seen_col, float* state,
                            int32_t* oob, hipStream_t s) {
    const int K0 = dims[0], N1 = dims[1], N2 = n_layers == 3 ? dims[2] : 0;
    const BlobPtrs w = blob_ptrs(packed, dims, n_layers);
    const int64_t npre = user_first ? rows : cols;
    const unsigned pblocks = (unsigned)(((npre + 31) / 32 + 3) / 4);
#define X(k0, n1, n2) \
    if (K0 == k0 && N1 == n1 && N2 == n2) \
        hipLaunchKernelGGL((mlp_prefix_kernel<k0, n1>), dim3(pblocks), dim3(256), 0, s, (const float*)tabA, rowsA, ldA, \
                           user_first ? user_ids : item_ids, npre, EA, w.Wp1, w.b1, state, oob);
    NCF_FUSED_INSTANCES(X)
#undef X
    a.tabB = (const float*)tabB; a.rowsB = rowsB; a.ldB = ldB;
    a.idxU = user_ids; a.idxI = item_ids;
    a.user_first = user_first ? 1 : 0;
    a.cols = cols; a.EA = EA;
    a.state = state;
    a.Wp1 = w.Wp1; a.Wp2 = w.Wp2; a.b2 = w.b2; a.wl = w.wl; a.bl = w.bl;
    a.seen_rowptr = seen_rowptr; a.seen_col = seen_col;
    a.oob = oob;
}


// What the two bodies below ask of a GMF term; the MLP entries have none (neumf.hip has NeuMF's).  extra_bytes: workspace behind the
// prefix state (a multiple of 16); check: the term's refusals, after the MLP operands'; prepare: launches what fills that workspace
// and sets the term's fields of the kernel arguments.
struct MlpNoGmf {
    typedef MtArgs TopkArgs;
    typedef MrArgs RankArgs;
    size_t extra_bytes(int64_t) const { return 0; }
    int check(const char*, int64_t, int) const { return NCF_OK; }
    template <class A>
    void prepare(A&, void*, int64_t, const int64_t*, int64_t, int32_t*, hipStream_t) const {}
};

template <class Gmf>
static size_t mlp_topk_ws_bytes(const char* what, const Gmf& gmf, int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims,
                                int k) {
    if (mt_check(rows, cols, k, what) != NCF_OK || rows == 0) return 0;
    if (!dims || (n_layers != 2 && n_layers != 3) || dims[1] < 32 || dims[1] % 32) return 0;
    return mlp_state_bytes(rows, cols, dims[1], user_first) + gmf.extra_bytes(rows) + topk_merge_bytes(mt_plan(rows, cols, k, nullptr));
}

// The body of ncf_mlp_topk and ncf_neumf_topk; `what` / `ws_what` name the entry point and its workspace query in the refusals.
template <class Gmf>
static int mlp_topk_run(const char* what, const char* ws_what, const Gmf& gmf, int dtype, const void* tabA, int64_t rowsA, int64_t ldA,
                        const void* tabB, int64_t rowsB, int64_t ldB, int EA, int EB, int user_first, const int64_t* user_ids,
                        const int64_t* item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims, const void* packed,
                        const int64_t* seen_rowptr, const int32_t* seen_col, int k, float* out_score, int32_t* out_idx, int32_t* out_count,
                        void* workspace, size_t workspace_bytes, int32_t* oob, hipStream_t s) {
    if (const int rc = mt_check(rows, cols, k, what)) return rc;
    if (const int rc = mlp_check_operands(what, dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, EA, EB, user_first, user_ids, item_ids, rows, cols,
                                          n_layers, dims, packed, 0, out_score && out_idx && out_count))
        return rc;
    if (const int rc = gmf.check(what, rows, user_first)) return rc;
    if (rows == 0) return NCF_OK;
    const int K0 = dims[0], N1 = dims[1], N2 = n_layers == 3 ? dims[2] : 0;
    int tile_cols;
    const TopkMerge p = mt_plan(rows, cols, k, &tile_cols);
    const size_t state_bytes = mlp_state_bytes(rows, cols, N1, user_first), extra = gmf.extra_bytes(rows);
    if (const int rc = topk_check_buffers(what, ws_what, seen_rowptr, seen_col, workspace, workspace_bytes,
                                          state_bytes + extra + topk_merge_bytes(p)))
        return rc;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + state_bytes + extra);
    typename Gmf::TopkArgs a{};
    mlp_prefix_pass(a, tabA, rowsA, ldA, tabB, rowsB, ldB, EA, user_first, user_ids, item_ids, rows, cols, n_layers, dims, packed,
                    seen_rowptr, seen_col, (float*)workspace, oob, s);
    gmf.prepare(a, (char*)workspace + state_bytes, rowsA, user_ids, rows, oob, s);
    a.tiles = (int)((cols + tile_cols - 1) / tile_cols); a.tile_cols = tile_cols; a.k = k; a.kp = p.kp;
    a.out_keys = keys; a.n_out = p.n1;
    for (int64_t r0 = 0; r0 < rows; r0 += p.chunk) {
        const int64_t nr = min(p.chunk, rows - r0);
        a.row0 = r0; a.nrows = nr;
        const unsigned blocks = (unsigned)((nr * a.tiles + kMtWaves - 1) / kMtWaves);
        mt_dispatch(K0, N1, N2, blocks, s, a);
        // merge levels over the fused level's kp keys per range; the last one sorts and writes (score from the key)
        topk_merge(p, keys, nullptr, 0, r0, nr, k, out_score, out_idx, out_count, s);
    }
    return check_launch(what);
}

template <class Gmf>
static size_t mlp_rank_ws_bytes(const char* what, const Gmf& gmf, int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims,
                                int64_t n_targets, int max_targets) {
    if (mr_check(rows, cols, max_targets, what) != NCF_OK || rows == 0 || n_targets < 0) return 0;
    if (!dims || (n_layers != 2 && n_layers != 3) || dims[1] < 32 || dims[1] % 32) return 0;
    return mlp_state_bytes(rows, cols, dims[1], user_first) + gmf.extra_bytes(rows) + rank_ws_bytes(n_targets, true);
}

// The body of ncf_mlp_rank and ncf_neumf_rank.  score_pairs(users, items, n, out): the entry's pair scorer over the (row, target)
// pairs, by position lists of the two id spaces; it returns a status.
template <class Gmf, class ScorePairs>
static int mlp_rank_run(const char* what, const char* ws_what, const Gmf& gmf, ScorePairs score_pairs, int dtype, const void* tabA,
                        int64_t rowsA, int64_t ldA, const void* tabB, int64_t rowsB, int64_t ldB, int EA, int EB, int user_first,
                        const int64_t* user_ids, const int64_t* item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims,
                        const void* packed, const int64_t* seen_rowptr, const int32_t* seen_col, const int64_t* tgt_rowptr,
                        const int32_t* tgt_col, int64_t n_targets, int max_targets, int32_t* rank, int32_t* ranked, void* workspace,
                        size_t workspace_bytes, int32_t* oob, int32_t* overflow, hipStream_t s) {
    if (const int rc = mr_check(rows, cols, max_targets, what)) return rc;
    if (const int rc = mlp_check_operands(what, dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, EA, EB, user_first, user_ids, item_ids, rows, cols,
                                          n_layers, dims, packed, n_targets, true))
        return rc;
    if (const int rc = gmf.check(what, rows, user_first)) return rc;
    if (rows == 0) return NCF_OK;
    const int K0 = dims[0], N1 = dims[1], N2 = n_layers == 3 ? dims[2] : 0;
    // N1 % 32 == 0 and the term's share: multiples of 16 bytes
    const size_t state_bytes = mlp_state_bytes(rows, cols, N1, user_first), extra = gmf.extra_bytes(rows);
    if (const int rc = rank_check_args(what, ws_what, rows, seen_rowptr, seen_col, tgt_rowptr, tgt_col, n_targets, rank, ranked, workspace,
                                       workspace_bytes, state_bytes + extra + rank_ws_bytes(n_targets, true)))
        return rc;
    const RankWs w = rank_ws_carve((char*)workspace + state_bytes + extra, n_targets, true);

    // the targets' own scores from the pair scorer, then their keys in order
    rank_expand(user_ids, item_ids, rows, cols, tgt_rowptr, tgt_col, n_targets, w, ranked, s);
    if (n_targets > 0) {
        if (const int rc = score_pairs(w.pair_user, w.pair_item, n_targets, w.pair_score)) return rc;
    }
    rank_prepare(nullptr, 0, w.pair_score, rows, cols, seen_rowptr, seen_col, tgt_rowptr, tgt_col, max_targets, true, w, rank, overflow, s);

    const int tile_cols = mr_tile_cols(rows, cols, max_targets);
    typename Gmf::RankArgs a{};
    mlp_prefix_pass(a, tabA, rowsA, ldA, tabB, rowsB, ldB, EA, user_first, user_ids, item_ids, rows, cols, n_layers, dims, packed,
                    seen_rowptr, seen_col, (float*)workspace, oob, s);
    gmf.prepare(a, (char*)workspace + state_bytes, rowsA, user_ids, rows, oob, s);
    a.row0 = 0; a.nrows = rows;
    a.tiles = (int)((cols + tile_cols - 1) / tile_cols); a.tile_cols = tile_cols;
    a.tgt_rowptr = tgt_rowptr; a.skey = w.skey; a.sperm = w.sperm;
    a.max_targets = max_targets; a.P = rank_slots(max_targets);
    a.rank = rank; a.ranked = ranked;
    const unsigned blocks = (unsigned)((rows * a.tiles + kMtWaves - 1) / kMtWaves);
    mr_dispatch(K0, N1, N2, max_targets == 1, blocks, s, a);
    return check_launch(what);
}

}  // namespace ncf
