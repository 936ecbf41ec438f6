// The GMF term of NeuMF (neumf.hip: ncf_neumf_score; mlp_topk.h with Args::kGmf: ncf_neumf_topk, ncf_neumf_rank), in ONE place: the
// pair scorer and the full-catalogue waves return the same bits because they run this code.  Internal: not part of the ABI.
//
// THE CONTRACT (include/ncf_abi.h, under ncf_neumf_score) for a pair with GMF rows p (user), q (item) and the weights w, D = 8 nS
// wide: lane half h in {0, 1} starts a_h = +0.f and, for s = 0 .. nS - 1 and j = 0 .. 3 with d = 8 s + 4 h + j,
//     t = fl(w[d] * p[d]);  v = fl(t * q[d]);  a_h = fl(a_h + v);          g = fl(a_0 + a_1)
// every product and sum rounded on its own.  The three functions that do arithmetic switch floating-point contraction off for their
// own statements (the pragma travels with the instructions when they are inlined), so no v_fma can take a product and a sum
// together; the file that includes this header keeps its flags, and its fmaf calls stay fused.
// g is never -0.0: a_h starts at +0.f, +0 + (-0) and an exact cancellation both give +0 in round-to-nearest, so a_h is never -0 and
// a_0 + a_1 is -0 only if both are.  An out-of-range id reads its side's row as zeros (gmf_row), which leaves a_h at +0.
#pragma once
#include "ncf_common.h"

namespace ncf {

constexpr int kGmfMaxD = 128;                        // D: a multiple of 8 in 8 .. kGmfMaxD

inline bool gmf_width_ok(int D) { return D >= 8 && D <= kGmfMaxD && D % 8 == 0; }

// a row chunk as loaded, or zeros for an id outside its table (a select, not a product: row 0 may hold anything)
__device__ __forceinline__ f32x4 gmf_row(f32x4 v, bool ok) { return ok ? v : f32x4{0.f, 0.f, 0.f, 0.f}; }

// t = fl(w * p) for one chunk of four
__device__ __forceinline__ f32x4 gmf_t(f32x4 w, f32x4 p) {
#pragma clang fp contract(off)
    return w * p;
}

// a_h after one chunk: v = fl(t * q), a = fl(a + v), j ascending
__device__ __forceinline__ float gmf_step(float a, f32x4 t, f32x4 q) {
#pragma clang fp contract(off)
    const f32x4 v = t * q;
    a = a + v[0];
    a = a + v[1];
    a = a + v[2];
    a = a + v[3];
    return a;
}

// g = fl(a_0 + a_1): the two lane halves hold a_0 and a_1 of the same pair (an addition commutes: both halves get g's bits)
__device__ __forceinline__ float gmf_join(float a) {
#pragma clang fp contract(off)
    return a + __shfl_xor(a, 32);
}

// g from a t row (t: the lane half's first chunk, any address space; the full-catalogue waves keep the user's in LDS) and the lane's
// item row qrow (the lane half's first chunk).  The first AHEAD chunks of qrow were loaded by the caller (qpre; a chunk past the
// row's end is a repeat that is not used), the others are loaded here.  AHEAD is given, not deduced: it may be 0.
template <int AHEAD>
__device__ __forceinline__ float gmf_dot_t(const float* t, const float* qrow, bool ok, int nS, const f32x4 (&qpre)[AHEAD > 0 ? AHEAD : 1]) {
    float a = 0.f;
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
        if (s < nS) a = gmf_step(a, *reinterpret_cast<const f32x4*>(t + 8 * s), gmf_row(qpre[s], ok));
    for (int s = AHEAD; s < nS; ++s)
        a = gmf_step(a, *reinterpret_cast<const f32x4*>(t + 8 * s), gmf_row(*reinterpret_cast<const f32x4*>(qrow + 8 * s), ok));
    return gmf_join(a);
}

// g of a pair from the rows themselves (w, prow, qrow: the lane half's first chunk of each): t is formed per chunk.  ppre / qpre as
// in gmf_dot_t.
template <int AHEAD>
__device__ __forceinline__ float gmf_dot_pair(const float* w, const float* prow, bool okp, const float* qrow, bool okq, int nS,
                                              const f32x4 (&ppre)[AHEAD], const f32x4 (&qpre)[AHEAD]) {
    float a = 0.f;
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
        if (s < nS)
            a = gmf_step(a, gmf_t(*reinterpret_cast<const f32x4*>(w + 8 * s), gmf_row(ppre[s], okp)), gmf_row(qpre[s], okq));
    for (int s = AHEAD; s < nS; ++s)
        a = gmf_step(a, gmf_t(*reinterpret_cast<const f32x4*>(w + 8 * s), gmf_row(*reinterpret_cast<const f32x4*>(prow + 8 * s), okp)),
                     gmf_row(*reinterpret_cast<const f32x4*>(qrow + 8 * s), okq));
    return gmf_join(a);
}

}  // namespace ncf
