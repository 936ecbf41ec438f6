// Shared pieces of the fp32 fused MLP scorers (mlp_fused.hip: ncf_score_fused, ncf_score_folded; mlp_partial.hip:
// ncf_score_fused_partial; mlp_topk.hip: ncf_mlp_topk, ncf_mlp_rank): the packed-blob layout written by ncf_mlp_pack, the list of
// compiled (K0, N1, N2) instances and the device stages every kernel of the family runs.  Internal: not part of the ABI.
#pragma once
#include "ncf_common.h"

namespace ncf {

// blob layout (floats): Wp1[N1*K0] b1[N1] (Wp2[N2*N1] b2[N2])? wl[Nlast] bl[1] pad
struct BlobLayout {
    size_t wp1, b1, wp2, b2, wl, bl, total;
};
static BlobLayout blob_layout(const int* dims, int n_layers) {
    BlobLayout L{};
    const size_t K0 = dims[0], N1 = dims[1];
    size_t off = 0;
    L.wp1 = off; off += N1 * K0;
    L.b1 = off; off += N1;
    size_t last = N1;
    if (n_layers == 3) {
        const size_t N2 = dims[2];
        L.wp2 = off; off += N2 * N1;
        L.b2 = off; off += N2;
        last = N2;
    }
    L.wl = off; off += last;
    L.bl = off; off += 4;  // keep 16-byte granularity
    L.total = off;
    return L;
}

#define NCF_FUSED_INSTANCES(X) \
    X(64, 256, 128) X(64, 256, 0) X(64, 128, 0) X(64, 128, 64) \
    X(128, 256, 128) X(128, 256, 0) X(128, 128, 0) X(128, 128, 64) \
    X(256, 256, 128) X(256, 256, 0) X(256, 128, 0)

// blob -> the pointers the kernels take (Wp2 / b2 NULL without a second hidden layer)
struct BlobPtrs {
    const float *Wp1, *b1, *Wp2, *b2, *wl, *bl;
};
static BlobPtrs blob_ptrs(const void* packed, const int* dims, int n_layers) {
    const BlobLayout L = blob_layout(dims, n_layers);
    const float* P = (const float*)packed;
    const bool l2 = n_layers == 3;
    return {P + L.wp1, P + L.b1, l2 ? P + L.wp2 : nullptr, l2 ? P + L.b2 : nullptr, P + L.wl, P + L.bl};
}

// The stages the fp32 MLP scorers share (mlp_fused.hip, mlp_partial.hip, mlp_topk.hip), in ONE place: the kernels return the same
// bits for the same pair because they run this code.
// Lane (m, h) of a 32-pair tile: the accumulator rows are neurons, register r of tile nt holds neuron 32nt + (r&3) + 8(r>>2) + 4h.
__device__ __forceinline__ f32x4 fused_ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// Tile nt of a bias, P row or prefix state (neuron order) into an accumulator, and back: four 16-byte chunks at
// src + 32nt + 8g + 4h (h = 0 where src already points at the lane half's chunk).
__device__ __forceinline__ void fused_load_tile(f32x16& acc, const float* src, int nt, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = fused_ldg4(src + 32 * nt + 8 * g + 4 * h);
        acc[4 * g + 0] = v[0]; acc[4 * g + 1] = v[1];
        acc[4 * g + 2] = v[2]; acc[4 * g + 3] = v[3];
    }
}
__device__ __forceinline__ void fused_store_tile(float* dst, const f32x16& acc, int nt, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(dst + 32 * nt + 8 * g + 4 * h) =
            f32x4{acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
}

// Pair prologue: this lane's row of `tab` for position p (id idx[p], p itself with idx NULL), offset to the lane half's chunk.
// Returns whether the id is in range.  An out-of-range id reads row 0, which fused_zmul's factor zeroes at USE; the caller raises
// the flag under its own condition.  The flag is the return value and the factor a function of its own on purpose: with a bool&
// or with the factor formed in here, score_fused_f32_kernel no longer compiles to the instructions it had.  The folded and the
// partial kernel (both ids are read before either is checked), mlp_topk_kernel and mlp_prefix_kernel (their register counts move)
// keep their own prologue.
__device__ __forceinline__ bool fused_row(int64_t p, const int64_t* idx, const float* tab, int64_t rows, int64_t ld, int h,
                                          const float*& row) {
    const int64_t i = idx ? idx[p] : p;
    const bool ok = (i >= 0) & (i < rows);
    row = tab + (ok ? i : 0) * ld + 4 * h;
    return ok;
}
__device__ __forceinline__ float fused_zmul(bool ok) { return ok ? 1.f : 0.f; }

// Layer 2: acc2 = b2 + W2 . relu(acc1); acc1's registers are the B operands.  Per k-step, MFMAs nt-major (4 dependent MFMAs per
// accumulator: the dependent latency of 32x32x2 equals its issue interval) and the next step's weight fragment of tile nt issued
// right behind tile nt's MFMAs.
template <int N1, int N2>
__device__ __forceinline__ void fused_layer2(const f32x16 (&acc1)[N1 / 32], f32x16 (&acc2)[N2 / 32], const float* b2,
                                             const float* Wp2, int lane) {
    constexpr int NT2 = N2 / 32, Q2 = N1 / 8;
    const int h = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt) fused_load_tile(acc2[nt], b2, nt, h);
    const f32x4* wp = reinterpret_cast<const f32x4*>(Wp2) + lane;
    f32x4 w[2][NT2];
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt) w[0][nt] = wp[nt * 64];
#pragma unroll
    for (int q = 0; q < Q2; ++q) {  // q = 4*kb + g : k-block kb of H1 (= tile kb of acc1), group g
        const int cur = q & 1, nxt = cur ^ 1;
        const int kb = q >> 2, g = q & 3;
        f32x4 hv;
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = fmaxf(acc1[kb][4 * g + j], 0.f);  // ReLU (util.py:15)
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][nt][j], hv[j], acc2[nt], 0, 0, 0);
            if (q + 1 < Q2) w[nxt][nt] = wp[((q + 1) * NT2 + nt) * 64];
        }
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMA
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// fused_layer2 for ncf_score_fused_partial (mlp_partial.hip) alone: the same steps (same loads, same MFMAs on the same operands in
// the same order), with the weight stream addressed from a scalar base.  In fused_layer2 every fragment's offset outgrows the load's
// immediate field and hipcc rebuilds a 64-bit vector address for it (a v_add_co_u32 / v_addc_co_u32 pair or a v_lshl_add_u64, with
// s_nop pads, between the MFMAs: 33 pairs per tile at 256-128).  Here the fragment of (q = 4 kb + g, nt) is read at
//   Wp2 + kb's bytes (scalar, one s_add_u32 / s_addc_u32 per k-block) + voff[g] (32-bit VGPR, set up once) + nt KiB (immediate),
// the SGPR-base form layer 1's loads take.  The two empty asm statements only keep hipcc from folding the parts back together; the
// scalar part passes through one as an offset, not as a pointer, so the loads stay global loads.  The other kernels keep
// fused_layer2: their instructions are pinned (see fused_row above), and DESIGN 4.20 has what this form measured.
// at_step(q) runs ahead of step q: a hook for the diagnostic stamp build, nothing otherwise.
struct fused_no_hook {
    __device__ __forceinline__ void operator()(int) const {}
};
template <int N1, int N2, class Hook = fused_no_hook>
__device__ __forceinline__ void fused_layer2_sbase(const f32x16 (&acc1)[N1 / 32], f32x16 (&acc2)[N2 / 32], const float* b2,
                                                   const float* Wp2, int lane, Hook at_step = Hook()) {
    constexpr int NT2 = N2 / 32, Q2 = N1 / 8;
    const int h = lane >> 5;
    const char* wb = reinterpret_cast<const char*>(Wp2);
    const char* kbase = wb;
    uint32_t voff[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        voff[g] = (uint32_t)lane * 16u + g * NT2 * 1024;
        asm("" : "+v"(voff[g]));
    }
    f32x4 w[2][NT2];
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt) {  // first-use order: tile nt of b2, then its step-0 fragment
        fused_load_tile(acc2[nt], b2, nt, h);
        w[0][nt] = *reinterpret_cast<const f32x4*>(kbase + voff[0] + nt * 1024);
    }
#pragma unroll
    for (int q = 0; q < Q2; ++q) {  // q = 4*kb + g : k-block kb of H1 (= tile kb of acc1), group g
        const int cur = q & 1, nxt = cur ^ 1;
        const int kb = q >> 2, g = q & 3;
        at_step(q);
        f32x4 hv;
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = fmaxf(acc1[kb][4 * g + j], 0.f);  // ReLU (util.py:15)
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][nt][j], hv[j], acc2[nt], 0, 0, 0);
            if (q + 1 < Q2) {
                if (nt == 0 && ((q + 1) & 3) == 0) {  // the next k-block's base
                    uint32_t koff = ((q + 1) >> 2) * 4 * NT2 * 1024;
                    asm("" : "+s"(koff));
                    kbase = wb + koff;
                }
                w[nxt][nt] = *reinterpret_cast<const f32x4*>(kbase + voff[(q + 1) & 3] + nt * 1024);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMA
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The 1-wide last layer without its bias: sum_n wl[n] * relu(acc[n]), per lane half over nt, g, j, then half 0 + half 1.
template <int NT>
__device__ __forceinline__ float fused_last_sum(const f32x16 (&acc)[NT], const float* wl, int lane) {
    const int h = lane >> 5;
    float partial = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 ww = fused_ldg4(wl + 32 * nt + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) partial = fmaf(ww[j], fmaxf(acc[nt][4 * g + j], 0.f), partial);
        }
    return partial + __shfl_xor(partial, 32);  // the two lane halves hold complementary neuron rows
}

// ... and with it: every lane returns its pair's score.
template <int NT>
__device__ __forceinline__ float fused_last_layer(const f32x16 (&acc)[NT], const float* wl, const float* bl, int lane) {
    return fused_last_sum(acc, wl, lane) + bl[0];
}

}  // namespace ncf
