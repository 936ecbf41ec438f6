// Shared pieces of the fp32 fused MLP scorers (mlp_fused.hip: ncf_score_fused; mlp_topk.hip: ncf_mlp_topk): the packed-blob
// layout written by ncf_mlp_pack and the list of compiled (K0, N1, N2) instances.  Internal: not part of the ABI.
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

// The part of the one-wave-per-tile fp32 scorers after layer 1 (score_fused_f32_kernel in mlp_fused.hip and
// score_fused_partial_f32_kernel in mlp_partial.hip), in ONE place: both kernels return the same bits because both run this.
// Lane (m, h) of a 32-pair tile: the accumulator rows are neurons, register r of tile nt holds neuron 32nt + (r&3) + 8(r>>2) + 4h.
__device__ __forceinline__ f32x4 fused_ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// Layer 2: acc2 = b2 + W2 . relu(acc1); acc1's registers are the B operands.  Per k-step, MFMAs nt-major and the next step's
// weight fragment of tile nt issued right behind tile nt's MFMAs.  PAIR / ABLATE: mlp_fused.hip's NCF_PAIR / NCF_ABLATE_LOADS.
template <int N1, int N2, bool PAIR = false, bool ABLATE = false>
__device__ __forceinline__ void fused_layer2(const f32x16 (&acc1)[N1 / 32], f32x16 (&acc2)[N2 / 32], const float* b2,
                                             const float* Wp2, int lane) {
    constexpr int NT2 = N2 / 32, Q2 = N1 / 8;
    const int h = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 bb = fused_ldg4(b2 + 32 * nt + 8 * g + 4 * h);
            acc2[nt][4 * g + 0] = bb[0]; acc2[nt][4 * g + 1] = bb[1];
            acc2[nt][4 * g + 2] = bb[2]; acc2[nt][4 * g + 3] = bb[3];
        }
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
        if (PAIR && NT2 % 2 == 0) {
#pragma unroll
            for (int nt = 0; nt < NT2; nt += 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][nt][j], hv[j], acc2[nt], 0, 0, 0);
                    acc2[nt + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][nt + 1][j], hv[j], acc2[nt + 1], 0, 0, 0);
                }
                if (q + 1 < Q2) {
                    w[nxt][nt] = ABLATE ? w[cur][nt] : wp[((q + 1) * NT2 + nt) * 64];
                    w[nxt][nt + 1] = ABLATE ? w[cur][nt + 1] : wp[((q + 1) * NT2 + nt + 1) * 64];
                }
            }
        } else {
#pragma unroll
            for (int nt = 0; nt < NT2; ++nt) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][nt][j], hv[j], acc2[nt], 0, 0, 0);
                if (q + 1 < Q2) w[nxt][nt] = ABLATE ? w[cur][nt] : wp[((q + 1) * NT2 + nt) * 64];
            }
        }
        if (!ABLATE) {
            if (PAIR && NT2 % 2 == 0) {
#pragma unroll
                for (int nt = 0; nt < NT2; nt += 2) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < NT2; ++nt) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The 1-wide last layer: bl + sum_n wl[n] * relu(acc[n]), per lane half over nt, g, j, then half 0 + half 1.  Every lane
// returns its pair's score.
template <int NT>
__device__ __forceinline__ float fused_last_layer(const f32x16 (&acc)[NT], const float* wl, const float* bl, int lane) {
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
    partial += __shfl_xor(partial, 32);  // the two lane halves hold complementary neuron rows
    return partial + bl[0];
}

}  // namespace ncf
