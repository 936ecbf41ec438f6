// The per-(edge, feature) message dropout mask of the graph kernels (include/ncf_abi.h, "THE MASK" under ncf_spmm_csr_dropout),
// shared by spmm.hip (forward and transposed aggregation) and gat.hip (the per-edge gradient of LightGAT's attention).
#pragma once
#include "ncf_common.h"

namespace ncf {

// Training-time dropout of the per-EDGE messages (the reference applies Dropout INSIDE the per-edge Linear, gnn_ncf.py:22-31,
// 91-93: message_e = coef_e * dropout(W(x[src_e])), one mask element per (edge, feature)).  The mask is never stored: element
// (edge id, feature) keeps iff a 16-bit slice of a counter-based hash of (seed, edge id, 16-byte chunk) reaches the threshold —
// the forward pass (CSR by destination) and its transpose (CSR by source, edge ids through `eid`) regenerate the same mask.
struct DropArgs {
    const int32_t* eid;   // edge id of each CSR entry (NULL: the entry's own position)
    uint32_t seed, thr;   // keep iff hash16 >= thr, thr = round(p * 65536)
    float scale;          // 1 / (1 - thr / 65536)
};
__device__ __forceinline__ f32x4 drop4(f32x4 v, uint32_t edge, int chunk, const DropArgs& d) {
    const uint32_t h0 = mix32(edge * 0x9E3779B1U ^ d.seed ^ (uint32_t)chunk * 0x85EBCA77U);
    const uint32_t h1 = mix32(h0 ^ 0x68E31DA4U);
    v[0] = (h0 & 0xFFFFU) >= d.thr ? v[0] * d.scale : 0.f;
    v[1] = (h0 >> 16) >= d.thr ? v[1] * d.scale : 0.f;
    v[2] = (h1 & 0xFFFFU) >= d.thr ? v[2] * d.scale : 0.f;
    v[3] = (h1 >> 16) >= d.thr ? v[3] * d.scale : 0.f;
    return v;
}

// (thr, scale) of a drop probability p in [0, 1): thr = (uint32)(p * 65536.f + 0.5f) clamped to 65535, scale = 65536 / (65536 - thr)
inline DropArgs drop_args(const int32_t* eid, uint32_t seed, float p) {
    DropArgs d;
    d.eid = eid;
    d.seed = seed;
    d.thr = (uint32_t)(p * 65536.f + 0.5f);
    if (d.thr > 65535u) d.thr = 65535u;
    d.scale = 65536.f / (float)(65536u - d.thr);
    return d;
}

}  // namespace ncf
