// The one owner of the drop rule and of the per-(entry, feature) mask hash (include/ncf_abi.h, "THE MASK" and "THE KEEP RULE"): the
// message dropout of spmm.hip and gat.hip, the hidden-layer and message dropout of attn.hip, the threshold of edge_keep.hip.
#pragma once
#include "ncf_common.h"

namespace ncf {

// THE DROP RULE.  A drop probability p becomes a 16-bit threshold: an element keeps iff its 16 hash bits are >= thr, and a kept
// element is multiplied by scale = 1 / (1 - thr / 65536).  p = 1 clamps to thr = 65535 (ncf_edge_keep accepts it; the entries that
// scale what they keep refuse p = 1 themselves).
struct DropThreshold { uint32_t thr; float scale; };
inline DropThreshold drop_threshold(float p) {
    uint32_t thr = (uint32_t)(p * 65536.f + 0.5f);
    if (thr > 65535u) thr = 65535u;
    return DropThreshold{thr, 65536.f / (float)(65536u - thr)};
}

// THE MASK HASH.  Two rounds of mix32 over (entry, 16-byte chunk, seed) give the four 16-bit slices of features 4 chunk .. 4 chunk + 3:
// h0 low, h0 high, h1 low, h1 high.
struct MaskHash { uint32_t h0, h1; };
__device__ __forceinline__ MaskHash mask_hash(uint32_t entry, int chunk, uint32_t seed) {
    const uint32_t h0 = mix32(entry * 0x9E3779B1U ^ seed ^ (uint32_t)chunk * 0x85EBCA77U);
    return MaskHash{h0, mix32(h0 ^ 0x68E31DA4U)};
}

// Training-time dropout of the per-EDGE messages (the reference applies Dropout INSIDE the per-edge Linear, gnn_ncf.py:22-31,
// 91-93: message_e = coef_e * dropout(W(x[src_e])), one mask element per (edge, feature)).  The mask is never stored: element
// (edge id, feature) keeps iff its slice of the mask hash reaches the threshold — the forward pass (CSR by destination) and its
// transpose (CSR by source, edge ids through `eid`) regenerate the same mask.
struct DropArgs {
    const int32_t* eid;   // edge id of each CSR entry (NULL: the entry's own position)
    uint32_t seed, thr;   // keep iff hash16 >= thr, thr = round(p * 65536)
    float scale;          // 1 / (1 - thr / 65536)
};
__device__ __forceinline__ f32x4 drop4(f32x4 v, uint32_t edge, int chunk, const DropArgs& d) {
    const MaskHash h = mask_hash(edge, chunk, d.seed);
    v[0] = (h.h0 & 0xFFFFU) >= d.thr ? v[0] * d.scale : 0.f;
    v[1] = (h.h0 >> 16) >= d.thr ? v[1] * d.scale : 0.f;
    v[2] = (h.h1 & 0xFFFFU) >= d.thr ? v[2] * d.scale : 0.f;
    v[3] = (h.h1 >> 16) >= d.thr ? v[3] * d.scale : 0.f;
    return v;
}

// the arguments of a drop probability p in [0, 1)
inline DropArgs drop_args(const int32_t* eid, uint32_t seed, float p) {
    const DropThreshold t = drop_threshold(p);
    return DropArgs{eid, seed, t.thr, t.scale};
}

}  // namespace ncf
