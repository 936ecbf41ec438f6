// Shared pieces of the per-row top-K (topk.hip: ncf_topk_rows; dot_topk.hip: ncf_dot_topk; mlp_topk.hip: ncf_mlp_topk): the key
// map, the wave-wide candidate helpers of the fused kernels, the tile select kernel, the launch plan.  See topk.hip for the
// ordering contract and the kernel shape.  Internal: not part of the ABI.
#pragma once
#include "ncf_common.h"

namespace ncf {

constexpr int kTopkThreads = 256;
constexpr int kTopkTile = 8192;                        // entries per workgroup: 32 per thread
constexpr int kTopkPer = kTopkTile / kTopkThreads;
constexpr int kTopkMaxK = 1024;
constexpr int64_t kTopkMaxCols = int64_t(1) << 24;
constexpr int64_t kTopkMaxRows = 65536;
constexpr size_t kTopkChunkBytes = size_t(256) << 20;  // workspace target: rows are processed in chunks that fit it

__device__ __forceinline__ uint32_t topk_map(float x) {
    uint32_t u = __float_as_uint(x);
    if (x != x) return 0u;                              // every NaN: below -inf
    if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inverse of topk_map for every key that is not a NaN's (0 maps back to a NaN); -0.0 comes back as +0.0
__device__ __forceinline__ float topk_unmap(uint32_t m) {
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((int)(uint32_t)v, m), hi = __shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

// (key >> top) == (ref >> top), with top = 64 meaning "no bits": true
__device__ __forceinline__ bool topk_high_eq(unsigned long long key, unsigned long long ref, int top) {
    return top >= 64 || ((key ^ ref) >> top) == 0;
}

// order this wave's LDS accesses (the LDS serves one wave's instructions in order; the fence keeps the compiler from moving
// memory operations across it)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// The largest key T with #{v >= T} >= keep over the wave's 4 x 64 keys (0 = empty; at least `keep` nonzero keys present).
__device__ unsigned long long wave_kth(const unsigned long long (&v)[4], int keep) {
    unsigned long long prefix = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = prefix | (1ull << bit);
        int c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) c += __popcll(__ballot(v[i] >= cand));
        if (c < keep) continue;
        prefix = cand;
        if (c == keep) {                 // exactly `keep` keys are >= cand: the smallest of them is the answer
            unsigned long long m = ~0ull;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (v[i] >= cand) m = min(m, v[i]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = min(m, shfl_xor_u64(m, o));
            return m;
        }
    }
    return prefix;
}

struct TopkShared {
    uint32_t hist[kTopkThreads / kWave][256];
    unsigned long long sel[kTopkMaxK];
    uint32_t bitmap[kTopkTile / 32];
    unsigned long long red_min[kTopkThreads / kWave], red_max[kTopkThreads / kWave];
    int red_cnt[kTopkThreads / kWave];
    int bin, above, cnt_bin, nsel;
};

// LEVEL0: `src` is the score matrix (row-major, leading dimension ld); else the previous level's keys (n_in per row).
// FINAL: write sorted (score, column) pairs + counts; else write kp keys per tile into out_keys (n_out per row).
template <bool LEVEL0, bool FINAL>
__global__ __launch_bounds__(kTopkThreads) void topk_tile_kernel(
    const float* __restrict__ scores, int64_t ld, int64_t cols, const int64_t* __restrict__ seen_rowptr, const int32_t* __restrict__ seen_col,
    const unsigned long long* __restrict__ in_keys, int64_t n_in, int tiles, int64_t row0, int k, int kp,
    unsigned long long* __restrict__ out_keys, int64_t n_out, float* __restrict__ out_score, int32_t* __restrict__ out_idx,
    int32_t* __restrict__ out_count) {
    __shared__ TopkShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x % tiles;
    const int64_t rloc = blockIdx.x / tiles, row = row0 + rloc;
    const int64_t t0 = (int64_t)tile * kTopkTile;
    const int64_t n_total = LEVEL0 ? cols : n_in;
    const int n = (int)min((int64_t)kTopkTile, n_total - t0);

    unsigned long long key[kTopkPer];
    if (LEVEL0) {
        const bool excl = seen_rowptr != nullptr;
        if (excl) {
            sh.bitmap[tid] = 0u;
            __syncthreads();
            const int64_t b = seen_rowptr[row], e = seen_rowptr[row + 1];
            for (int64_t p = b + tid; p < e; p += kTopkThreads) {
                const int64_t c = (int64_t)seen_col[p] - t0;   // duplicates and ids outside [0, cols) fall out here or do nothing
                if (c >= 0 && c < n) atomicOr(&sh.bitmap[c >> 5], 1u << (c & 31));
            }
            __syncthreads();
        }
        const float* src = scores + row * ld + t0;
        const bool vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;   // e is a multiple of 4: every quad is then aligned
#pragma unroll
        for (int it = 0; it < kTopkPer / 4; ++it) {
            const int e = it * (kTopkThreads * 4) + tid * 4;
            float v[4];
            if (vec && e + 3 < n) {
                const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + e));
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = e + j < n ? src[e + j] : 0.f;
            }
            const uint32_t bits = excl ? sh.bitmap[e >> 5] >> (e & 31) : 0u;   // e % 4 == 0: the 4 bits are in one word
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = e + j < n && !((bits >> j) & 1u);
                const uint32_t col = (uint32_t)(t0 + e + j);
                key[it * 4 + j] = ok ? ((unsigned long long)topk_map(v[j]) << 32) | (0xFFFFFFFFu - col) : 0ull;
            }
        }
    } else {
        const unsigned long long* src = in_keys + rloc * n_in + t0;       // n_in and t0 even: 16-byte aligned pairs
#pragma unroll
        for (int it = 0; it < kTopkPer / 2; ++it) {
            const int e = it * (kTopkThreads * 2) + tid * 2;
            if (e < n) {
                const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + e));
                key[it * 2] = ((unsigned long long)q[1] << 32) | q[0];
                key[it * 2 + 1] = ((unsigned long long)q[3] << 32) | q[2];
            } else {
                key[it * 2] = key[it * 2 + 1] = 0ull;
            }
        }
    }

    // ---- valid count, min / max of the valid keys
    unsigned long long kmin = ~0ull, kmax = 0ull;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < kTopkPer; ++i) {
        if (key[i]) {
            ++cnt;
            kmin = min(kmin, key[i]);
            kmax = max(kmax, key[i]);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        cnt += __shfl_xor(cnt, m);
        kmin = min(kmin, shfl_xor_u64(kmin, m));
        kmax = max(kmax, shfl_xor_u64(kmax, m));
    }
    if (lane == 0) {
        sh.red_cnt[wave] = cnt;
        sh.red_min[wave] = kmin;
        sh.red_max[wave] = kmax;
    }
    if (tid == 0) sh.nsel = 0;
    __syncthreads();
    cnt = 0;
    kmin = ~0ull;
    kmax = 0ull;
#pragma unroll
    for (int w = 0; w < kTopkThreads / kWave; ++w) {
        cnt += sh.red_cnt[w];
        kmin = min(kmin, sh.red_min[w]);
        kmax = max(kmax, sh.red_max[w]);
    }

    // ---- radix select: thr = the smallest key that is selected (every valid key >= thr is, and there are min(k, cnt) of them)
    unsigned long long thr = 1ull;
    if (cnt > k) {
        int top = 64 - __builtin_clzll(kmin ^ kmax);    // bits [top, 64) are common to every valid key (kmin != kmax: cnt > 1)
        unsigned long long prefix = kmax;
        int need = k;
        while (true) {
            const int shift = max(top - 8, 0);
            const uint32_t dmask = (1u << (top - shift)) - 1u;
#pragma unroll
            for (int i = tid; i < (kTopkThreads / kWave) * 256; i += kTopkThreads) (&sh.hist[0][0])[i] = 0u;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kTopkPer; ++i)
                if (key[i] && topk_high_eq(key[i], prefix, top)) atomicAdd(&sh.hist[wave][(uint32_t)(key[i] >> shift) & dmask], 1u);
            __syncthreads();
            if (wave == 0) {
                // lane l holds bins 255-4l .. 252-4l (descending); an inclusive scan over lanes finds the bin of the need-th key
                uint32_t c[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int b = 255 - 4 * lane - q;
                    c[q] = sh.hist[0][b] + sh.hist[1][b] + sh.hist[2][b] + sh.hist[3][b];
                    s += c[q];
                }
                uint32_t incl = s;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(incl, d);
                    if (lane >= d) incl += o;
                }
                const uint32_t excl = incl - s;
                if (excl < (uint32_t)need && (uint32_t)need <= incl) {
                    uint32_t run = excl;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (run < (uint32_t)need && (uint32_t)need <= run + c[q]) {
                            sh.bin = 255 - 4 * lane - q;
                            sh.above = (int)run;
                            sh.cnt_bin = (int)c[q];
                        }
                        run += c[q];
                    }
                }
            }
            __syncthreads();
            const int bin = sh.bin, above = sh.above, cnt_bin = sh.cnt_bin;
            __syncthreads();                            // every thread has read them before the next pass overwrites
            const unsigned long long lowmask = top >= 64 ? ~0ull : ((1ull << top) - 1ull);
            prefix = (prefix & ~lowmask) | ((unsigned long long)bin << shift);
            need -= above;
            top = shift;
            if (cnt_bin == need || top == 0) break;     // keys are unique: at top == 0 the bucket is one key
        }
        thr = top == 0 ? prefix : (prefix & ~((1ull << top) - 1ull));
    }

    // ---- gather the selected keys in LDS
#pragma unroll
    for (int i = 0; i < kTopkPer; ++i) {
        if (key[i] && key[i] >= thr) {
            const int p = atomicAdd(&sh.nsel, 1);
            if (p < kTopkMaxK) sh.sel[p] = key[i];
        }
    }
    __syncthreads();
    const int nsel = min(sh.nsel, k);

    if (!FINAL) {
        unsigned long long* dst = out_keys + rloc * n_out + (int64_t)tile * kp;
        for (int s = tid; s < kp; s += kTopkThreads) dst[s] = s < nsel ? sh.sel[s] : 0ull;
        return;
    }
    // ---- bitonic sort (descending) of the survivors, padded with 0 keys to a power of two
    int P = 2;
    while (P < nsel) P <<= 1;
    for (int s = nsel + tid; s < P; s += kTopkThreads) sh.sel[s] = 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += kTopkThreads) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = sh.sel[lo], b = sh.sel[hi];
                if ((a < b) == desc) {
                    sh.sel[lo] = b;
                    sh.sel[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const float* srow = scores ? scores + row * ld : nullptr;
    for (int s = tid; s < k; s += kTopkThreads) {
        if (s < nsel) {
            const uint32_t col = 0xFFFFFFFFu - (uint32_t)sh.sel[s];
            out_idx[row * k + s] = (int32_t)col;
            out_score[row * k + s] = scores ? srow[col] : topk_unmap((uint32_t)(sh.sel[s] >> 32));
        } else {
            out_idx[row * k + s] = -1;
            out_score[row * k + s] = -__builtin_inff();
        }
    }
    if (tid == 0) out_count[row] = nsel;
}

// The launch plan of one row: tiles per level (level 0 over the columns, then over kp * tiles of the previous level).
struct TopkPlan {
    int levels;
    int64_t tiles[8];
    int kp;
    int64_t n1, n2;          // keys per row in the two ping-pong buffers (level 0 -> A: n1, level 1 -> B: n2)
    int64_t chunk;           // rows per chunk
};

static TopkPlan topk_plan(int64_t rows, int64_t cols, int k) {
    TopkPlan p{};
    p.kp = (k + 1) & ~1;
    int64_t n = cols;
    p.levels = 0;
    while (true) {
        const int64_t t = (n + kTopkTile - 1) / kTopkTile;
        p.tiles[p.levels++] = t;
        if (t == 1) break;
        n = t * p.kp;
    }
    p.n1 = p.levels > 1 ? p.tiles[0] * p.kp : 0;
    p.n2 = p.levels > 2 ? p.tiles[1] * p.kp : 0;
    const int64_t per_row = (p.n1 + p.n2) * 8;
    p.chunk = per_row ? max((int64_t)1, min(rows, (int64_t)(kTopkChunkBytes / per_row))) : rows;
    return p;
}

static bool topk_shape_ok(int64_t rows, int64_t cols, int k) {
    return rows >= 0 && rows <= kTopkMaxRows && cols >= 1 && cols <= kTopkMaxCols && k >= 1 && k <= kTopkMaxK;
}

}  // namespace ncf
