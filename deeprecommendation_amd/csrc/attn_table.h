// The softmax of one column of the logit table over one user's rated set, as one wave computes it: the statistics (m, l) that
// attn_explain.hip's weights and attn_stats.hip's tables are both made of.  ncf_attn_logits' table ST (attn_cross.hip) holds the
// logit of (rated item r, candidate c) at ST[r, c]; entry e of the user's CSR row [beg, end) contributes s_e = ST[col_e, c], or
// -inf when col_e is outside [0, I_r) (a masked entry).  Lane l owns the entries beg + l, beg + l + 64, ... in every pass; the
// first kTableCache logits stay in the wave's LDS strip between the passes (a lane reads back only what it wrote, so no fence is
// needed; longer rows look the rest up again).  Every order is fixed: equal inputs give equal bits, in every kernel that calls this.
// Internal.
#pragma once
#include "attn_util.h"

namespace ncf {

constexpr int kTableCache = 512;       // logits kept per wave between the passes (a multiple of 64)

struct TableColumn {
    const float* __restrict__ stc;     // ST + c: the candidate's column
    int64_t ldst, Ir;
    const int32_t* __restrict__ col;
    int64_t beg, end;                  // the user's entries; beg == end for a dead pair
    float* cache;                      // the wave's strip of kTableCache floats
    int lane;

    __device__ __forceinline__ float logit(int cc) const { return (cc >= 0 && cc < Ir) ? stc[(int64_t)cc * ldst] : -INFINITY; }

    // pass 1: looks every logit up, fills the strip; returns m = the exact maximum (fmaxf, then the xor butterfly), -inf for an
    // empty or fully masked row, an all -inf column or a dead pair
    __device__ __forceinline__ float max() const {
        float m = -INFINITY;
        for (int64_t e0 = beg; e0 < end; e0 += kWave) {
            const int64_t e = e0 + lane;
            const float s = e < end ? logit(col[e]) : -INFINITY;
            if (e0 - beg < kTableCache) cache[e0 - beg + lane] = s;
            m = fmaxf(m, s);
        }
        return wave_max(m);
    }

    // the logit of entry e = e0 + lane < end after pass 1; the branch is wave-uniform
    __device__ __forceinline__ float cached(int64_t e0, int64_t e) const {
        return e0 - beg < kTableCache ? cache[e - beg] : logit(col[e]);
    }

    // pass 2: l = the sum of exp_le0(s_e - m), per lane in entry order, then the xor butterfly 32, 16, .., 1 (commutative at every
    // step: all lanes hold the same bits); skipped (l = 0) when m = -inf
    __device__ __forceinline__ float denominator(float m) const {
        float l = 0.f;
        if (m != -INFINITY)
            for (int64_t e0 = beg; e0 < end; e0 += kWave) {
                const int64_t e = e0 + lane;
                if (e < end) l += exp_le0(cached(e0, e) - m);      // a masked entry: exp_le0(-inf) = 0
            }
        return wave_sum(l);
    }
};

}  // namespace ncf
