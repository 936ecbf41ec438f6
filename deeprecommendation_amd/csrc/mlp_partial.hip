// Partial first layer of the fp32 fused scorer — ncf_layer1_partial + ncf_score_fused_partial, gfx950.
//
// ncf_score_fused (mlp_fused.hip) computes every layer-1 neuron as ONE chain of v_mfma_f32_32x32x2_f32 that starts from
// b1[n] and runs over the k-groups q = 0 .. K0/8-1 in ascending order, and cat(A, B) puts table A's EA columns first.
// So after the first EA/8 groups each accumulator holds an fp32 value that depends on the row of table A, W1 and b1 only,
// not on the pair.  ncf_layer1_partial computes that value once per weight version for every row of A — the same MFMA
// instructions on the same packed fragments in the same order, with the row of A in the pair's place — and stores it as
// P[rowsA + 1][N1] in natural neuron order.  ncf_score_fused_partial starts each pair's accumulators from P[ia] and runs
// layer 1 over table B's groups only; layer 2 runs the fused kernel's steps with its weight stream addressed from a scalar base
// (fused_layer2_sbase, mlp_fused.h), the 1-wide layer is the fused kernel's.  An accumulator register
// stored and loaded back is the same fp32 value, so the scores are bit-identical to ncf_score_fused (denormals, NaN and
// signed zeros included).  At 128-256-128-1 a 32-pair tile issues 768 MFMAs instead of 1024.
// Row rowsA of P is what the fused kernel computes for an out-of-range A id (row 0 multiplied by zero at use); a bad id
// reads it.
#ifndef NCF_PART_STAMP
#define NCF_PART_STAMP 0    // 1: diagnostic build, clock readings at six points of the scoring kernel (tools/ab_partial.py --stamp)
#endif
#if NCF_PART_STAMP
#define NCF_STAMP(st, i)                                                                                            \
    do {                                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(st[2 * (i)]), "=s"(st[2 * (i) + 1])::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    } while (0)
#else
#define NCF_STAMP(st, i) do { } while (0)
#endif
#include "mlp_fused.h"

#ifndef NCF_PART_WD
#define NCF_PART_WD 8       // layer-1 weight fragments in flight (ring depth, steps of 4 MFMAs)
#endif
#ifndef NCF_PART_PF
#define NCF_PART_PF 2       // P tiles (32 neurons = one 128-byte line per pair) requested ahead of their first MFMA
#endif
#ifndef NCF_PART_LDS
#define NCF_PART_LDS 1      // 1: instances whose layer-1 image fits twice in a CU's LDS read it from there; 0: all stream it (A/B builds)
#endif
#ifndef NCF_PART_LDS_PF
#define NCF_PART_LDS_PF 2   // P tiles requested ahead in the LDS form (the only loads on its vector-memory queue); swept 1 .. 8
#endif
#ifndef NCF_PART_SBASE
#define NCF_PART_SBASE 1    // 1: layer 2's weight stream is addressed from a scalar base (fused_layer2_sbase); 0: fused_layer2 (A/B builds)
#endif
#ifndef NCF_PART_HYBRID_MAX_PERMILLE
#define NCF_PART_HYBRID_MAX_PERMILLE 500  // a batch, or a ragged last round, of at most this share of a round goes to ncf_score_fused
#endif

namespace ncf {

// ---------------------------------------------------------------------------------------------------------------
// Build: one wave = 32 rows of A, each in a pair's place of the fused kernel's layer 1, groups q < QA only.  The prefix pass of
// ncf_mlp_topk (mlp_prefix_kernel, mlp_topk.hip) is the same computation without the look-ahead: this loop, which asks for the next
// group's fragments and row chunk ahead of a group's MFMAs, measured 2.5 % slower there at 1 M rows, so both stay.
struct PartialBuildArgs {
    const float* tabA; int64_t rowsA; int64_t ldA; int QA;
    const float* Wp1; const float* b1;
    float* P; int64_t ldP;
};

template <int N1>
__global__ __launch_bounds__(256) void layer1_partial_kernel(PartialBuildArgs a) {
    constexpr int NT1 = N1 / 32;
    const int lane = threadIdx.x & 63;
    const int m = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t rows = a.rowsA + 1;
    if (tile * 32 >= rows) return;
    const int64_t r = tile * 32 + m;
    const bool ok = r < a.rowsA;    // row rowsA (and the lanes past it): the fused kernel's out-of-range id = row 0 times 0
    const float* rowA = a.tabA + (ok ? r : 0) * a.ldA + 4 * h;
    const float zA = fused_zmul(ok);

    f32x16 acc[NT1];
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) fused_load_tile(acc[nt], a.b1, nt, h);
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.Wp1) + lane;  // + (q*NT1 + nt)*64
    f32x4 w[NT1], x;
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) w[nt] = wp[nt * 64];
    x = fused_ldg4(rowA);
    for (int q = 0; q < a.QA; ++q) {
        f32x4 wn[NT1], xn;
        if (q + 1 < a.QA) {
#pragma unroll
            for (int nt = 0; nt < NT1; ++nt) wn[nt] = wp[((q + 1) * NT1 + nt) * 64];
            xn = fused_ldg4(rowA + 8 * (q + 1));
        }
        const f32x4 xb = x * zA;  // the fused kernel's use-time zeroing of an out-of-range row
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nt][j], xb[j], acc[nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt) w[nt] = wn[nt];
        x = xn;
    }
    if (r >= rows) return;
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) fused_store_tile(a.P + r * a.ldP, acc[nt], nt, h);
}

// ---------------------------------------------------------------------------------------------------------------
// Scoring from P.  Layer 1 runs nt-outer: accumulator tile nt starts from P tile nt and takes its QB*4 dependent MFMAs in
// one go (the chain of every accumulator is the fused kernel's: ascending q, then j).  The pair's QB chunks of table B
// stay in registers for all tiles; the weight fragment of (group qa + t, tile nt) is streamed through a ring of WD
// fragments (streaming form) or read from an LDS image (LDS form, below); P tile nt + PF is loaded straight into the
// not-yet-live acc1[nt + PF] at the end of tile nt.
struct PartialArgs {
    const float* P; int64_t rowsA; int64_t ldP;
    const float* tabB; int64_t rowsB; int64_t ldB;
    const int64_t* idxA; const int64_t* idxB;
    int64_t B; int QA;
    const float* Wp1; const float* Wp2; const float* b2;
    const float* wl; const float* bl;
    float* out; int32_t* oob;
#if NCF_PART_STAMP
    unsigned long long* stamps;   // diagnostic build only: 12 readings per wave, a buffer of their own
#endif
};

#if NCF_PART_STAMP
// Diagnostic build: shader clock and 100 MHz reference clock at six points of the kernel.  Nothing of it is compiled
// into the shipped library.
static unsigned long long* g_stamp_buf = nullptr;
extern "C" void ncf_partial_stamp_buffer(void* buf) { g_stamp_buf = (unsigned long long*)buf; }
#endif

// LDS form (LDS = true, partial_in_lds): table B's half of Wp1 is copied once per workgroup into an LDS image in step order
// (step s = nt*QB + t at wlds[s*64 + lane]: one conflict-free ds_read_b128 per step, counted on lgkmcnt), so the vector-memory
// queue holds the P gathers alone in the loop and a P tile asked PF tiles ahead really has PF tiles of MFMAs to arrive in: vmcnt
// retires in issue order, and in the streaming form every weight wait also waits for the P tile issued before that fragment.
// The fill loads are issued before every P load (writing them to LDS never waits for HBM) and the one barrier is reached by
// every wave of the workgroup, dead ones included; nothing after it synchronises.
constexpr bool partial_in_lds(int QB, int N1) { return NCF_PART_LDS && QB * (N1 / 32) <= 80; }  // KiB; two workgroups share 160

template <int QB, int N1, int N2, bool LDS>
__global__ __launch_bounds__(256, 2) void score_fused_partial_f32_kernel(PartialArgs a) {
    constexpr int NT1 = N1 / 32;
    constexpr int S = NT1 * QB;                                      // layer-1 steps of 4 MFMAs, nt-major
    constexpr int WD0 = (QB >= 16 && N1 >= 256) ? 4 : NCF_PART_WD;  // 64 VGPRs of table B leave room for 4 (else scratch)
    constexpr int WD = LDS ? 2 : (WD0 < S ? WD0 : S);
    constexpr int PF0 = LDS ? NCF_PART_LDS_PF : NCF_PART_PF;
    constexpr int PF = PF0 < 1 ? 1 : (PF0 < NT1 ? PF0 : NT1);
    constexpr int FILL = LDS ? S / 4 : 1;                            // fragments each of the 4 waves copies into the image
    __shared__ __attribute__((aligned(16))) f32x4 wlds[LDS ? S * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const bool live = tile * 32 < a.B;
#if NCF_PART_STAMP
    unsigned long long st[12];
#endif
    NCF_STAMP(st, 0);
    if (!LDS && !live) return;  // whole wave exits together; the LDS form leaves behind its barrier
    const int64_t p = tile * 32 + m;
    const int64_t pc = p < a.B ? p : a.B - 1;

    const int64_t ia = a.idxA ? a.idxA[pc] : pc;
    const int64_t ib = a.idxB ? a.idxB[pc] : pc;
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.Wp1) + (int64_t)a.QA * NT1 * 64 + lane;
    auto wfrag = [&](int s) { return wp[((s % QB) * NT1 + s / QB) * 64]; };  // step s = nt*QB + t: group qa + t, tile nt
    f32x4 fill[FILL];
    if constexpr (LDS) {  // steps 4i + wave; QB % 4 == 0, so (4i + wave) / QB = 4i / QB
#pragma unroll
        for (int i = 0; i < FILL; ++i) fill[i] = wp[(((4 * i) % QB + wave) * NT1 + (4 * i) / QB) * 64];
    }
    const bool okA = (ia >= 0) & (ia < a.rowsA), okB = (ib >= 0) & (ib < a.rowsB);
    if (!(okA & okB) && a.oob && live) *a.oob = 1;
    // Not fused_row's prologue: both ids are read ahead of the fill loads, and a bad A id reads the sentinel row, not row 0.
    const float* prow = a.P + (okA ? ia : a.rowsA) * a.ldP + 4 * h;
    const float* rowB = a.tabB + (okB ? ib : 0) * a.ldB + 4 * h;
    const float zB = okB ? 1.f : 0.f;

    f32x16 acc1[NT1];
    auto load_p = [&](int nt) { fused_load_tile(acc1[nt], prow, nt, 0); };  // prow carries the lane half's 4h already
    f32x4 w[WD], x[QB];
    // Issue order = first-use order: the in-order vmcnt wait for a fragment never waits for a younger load.
    load_p(0);
    if constexpr (!LDS) {
#pragma unroll
        for (int s = 0; s < WD - 1; ++s) w[s] = wfrag(s);
    }
#pragma unroll
    for (int t = 0; t < QB; ++t) x[t] = fused_ldg4(rowB + 8 * t);
#pragma unroll
    for (int nt = 1; nt < PF; ++nt) load_p(nt);
    const f32x4* wq = wlds + lane;  // + s*64
    if constexpr (LDS) {
#pragma unroll
        for (int i = 0; i < FILL; ++i) wlds[(4 * i + wave) * 64 + lane] = fill[i];
        __syncthreads();
        if (!live) return;
        NCF_STAMP(st, 1);
        w[0] = wq[0];
        w[1] = wq[64];
        __builtin_amdgcn_sched_barrier(0);  // both reads stay above tile 0: its "1 DS read" groups are for steps 2 ..
    }
#pragma unroll
    for (int nt = 0; nt < NT1; ++nt) {
#pragma unroll
        for (int t = 0; t < QB; ++t) {
            const int s = nt * QB + t;
            const f32x4 xb = x[t] * zB;  // zero an out-of-range row at USE time, as the fused kernel does
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s % WD][j], xb[j], acc1[nt], 0, 0, 0);
            if constexpr (LDS) {  // the fragment of step s + 2 into the quad step s has just read: a full step of cover
                if (s + 2 < S) w[s % 2] = wq[(s + 2) * 64];
            } else {
                if (s + WD - 1 < S) w[(s + WD - 1) % WD] = wfrag(s + WD - 1);
            }
        }
        if (nt + PF < NT1) load_p(nt + PF);
#pragma unroll
        for (int t = 0; t < QB; ++t) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                 // 4 MFMA
            __builtin_amdgcn_sched_group_barrier(LDS ? 0x100 : 0x020, 1, 0);  // 1 DS / VMEM read (a later fragment)
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);      // the P tile
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- layer 2 and the 1-wide layer: the steps of ncf_score_fused's kernel (mlp_fused.h), layer 2's weights from a scalar base ----
    NCF_STAMP(st, 2);
    float score;
    if constexpr (N2 > 0) {
        f32x16 acc2[N2 / 32];
#if NCF_PART_STAMP
        fused_layer2_sbase<N1, N2>(acc1, acc2, a.b2, a.Wp2, lane, [&](int q) { if (q == 4) NCF_STAMP(st, 3); });  // 16 MFMAs in
#elif NCF_PART_SBASE
        fused_layer2_sbase<N1, N2>(acc1, acc2, a.b2, a.Wp2, lane);
#else
        fused_layer2<N1, N2>(acc1, acc2, a.b2, a.Wp2, lane);
#endif
        NCF_STAMP(st, 4);
        score = fused_last_layer(acc2, a.wl, a.bl, lane);
    } else {
        score = fused_last_layer(acc1, a.wl, a.bl, lane);
    }
    if (h == 0 && p < a.B) a.out[p] = score;
#if NCF_PART_STAMP
    __builtin_amdgcn_s_waitcnt(0);   // the score is stored: the exit reading covers it
    NCF_STAMP(st, 5);
    if (lane == 0 && a.stamps) {
#pragma unroll
        for (int i = 0; i < 12; ++i) a.stamps[tile * 12 + i] = st[i];
    }
#endif
}

template <int QB, int N1, int N2>
static void launch_partial(const PartialArgs& a, hipStream_t s) {
    const int64_t tiles = (a.B + 31) / 32;
    hipLaunchKernelGGL((score_fused_partial_f32_kernel<QB, N1, N2, partial_in_lds(QB, N1)>), dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, a);
}

// The reachable instances: QB = EB / 8 in {4, 8, 12, 16} with 0 < EB < K0 for a (K0, N1, N2) of NCF_FUSED_INSTANCES.  (N1, N2) =
// (128, 64) exists at K0 = 64 and 128 only, so EB = 128 (QB = 16) cannot reach it.
#define NCF_PARTIAL_INSTANCES(X) \
    X(4, 256, 128) X(8, 256, 128) X(12, 256, 128) X(16, 256, 128) \
    X(4, 256, 0) X(8, 256, 0) X(12, 256, 0) X(16, 256, 0) \
    X(4, 128, 0) X(8, 128, 0) X(12, 128, 0) X(16, 128, 0) \
    X(4, 128, 64) X(8, 128, 64) X(12, 128, 64)

static bool partial_dispatch(int QB, int N1, int N2, const PartialArgs* a, hipStream_t s) {
#define X(qb, n1, n2) \
    if (QB == qb && N1 == n1 && N2 == n2) { if (a) launch_partial<qb, n1, n2>(*a, s); return true; }
    NCF_PARTIAL_INSTANCES(X)
#undef X
    return false;
}

static bool partial_shape_ok(int dtype, int EA, int EB, int n_layers, const int* dims) {
    if (dtype != NCF_F32 || !dims || EA <= 0 || EB <= 0 || EA % 8 || EB % 8) return false;
    if (!ncf_score_fused_supported(dtype, EA, EB, n_layers, dims)) return false;   // a (K0, N1, N2) fused instance
    return partial_dispatch(EB / 8, dims[1], n_layers == 3 ? dims[2] : 0, nullptr, nullptr);
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_score_fused_partial_supported(int dtype, int EA, int EB, int n_layers, const int* dims) {
    return partial_shape_ok(dtype, EA, EB, n_layers, dims) ? 1 : 0;
}

extern "C" int ncf_score_fused_partial_in_lds(int dtype, int EA, int EB, int n_layers, const int* dims) {
    return partial_shape_ok(dtype, EA, EB, n_layers, dims) && partial_in_lds(EB / 8, dims[1]) ? 1 : 0;
}

extern "C" int ncf_layer1_partial(int dtype, const void* tabA, int64_t rowsA, int64_t ldA, int EA, int EB, int n_layers,
                                  const int* dims, const void* packed, void* P, int64_t ldP, ncf_stream_t stream) {
    if (!partial_shape_ok(dtype, EA, EB, n_layers, dims))
        return fail(NCF_EUNSUPPORTED, "ncf_layer1_partial: no partial kernel for dtype=%d EA=%d EB=%d layers=%d", dtype, EA, EB, n_layers);
    const int N1 = dims[1];
    if (rowsA < 1 || !tabA || !packed || !P) return fail(NCF_EINVAL, "ncf_layer1_partial: bad argument");
    if (ldA < EA || ldA % 4 || ldP < N1 || ldP % 4 || !aligned16(tabA) || !aligned16(P) || !aligned16(packed))
        return fail(NCF_EINVAL, "ncf_layer1_partial: tables must be 16-byte aligned with ld %% 4 == 0");
    const BlobPtrs w = blob_ptrs(packed, dims, n_layers);
    PartialBuildArgs a;
    a.tabA = (const float*)tabA; a.rowsA = rowsA; a.ldA = ldA; a.QA = EA / 8;
    a.Wp1 = w.Wp1; a.b1 = w.b1;
    a.P = (float*)P; a.ldP = ldP;
    const int64_t tiles = (rowsA + 1 + 31) / 32;
    const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
    if (N1 == 256) hipLaunchKernelGGL(layer1_partial_kernel<256>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(layer1_partial_kernel<128>, grid, block, 0, (hipStream_t)stream, a);
    return check_launch("ncf_layer1_partial");
}

extern "C" int ncf_score_fused_partial(int dtype, const void* P, int64_t ldP, const void* tabA, int64_t rowsA, int64_t ldA,
                                       const void* tabB, int64_t rowsB, int64_t ldB, const int64_t* idxA, const int64_t* idxB,
                                       int64_t B, int EA, int EB, int n_layers, const int* dims, const void* packed, float* out,
                                       int32_t* oob, ncf_stream_t stream) {
    if (!partial_shape_ok(dtype, EA, EB, n_layers, dims))
        return fail(NCF_EUNSUPPORTED, "ncf_score_fused_partial: no partial kernel for dtype=%d EA=%d EB=%d layers=%d", dtype, EA, EB, n_layers);
    if (B == 0) return NCF_OK;
    const int N1 = dims[1];
    if (B < 0 || rowsA < 1 || !P || !tabA || !tabB || !packed || !out) return fail(NCF_EINVAL, "ncf_score_fused_partial: bad argument");
    if (ldA < EA || ldB < EB || ldP < N1 || ldA % 4 || ldB % 4 || ldP % 4 || !aligned16(tabA) || !aligned16(tabB) || !aligned16(P) ||
        !aligned16(packed))
        return fail(NCF_EINVAL, "ncf_score_fused_partial: tables must be 16-byte aligned with ld %% 4 == 0");
    hipStream_t s = (hipStream_t)stream;
    auto plain = [&](int64_t off, int64_t n) {   // the same pairs through ncf_score_fused: the same bits
        return ncf_score_fused(dtype, tabA, rowsA, ldA, tabB, rowsB, ldB, idxA ? idxA + off : nullptr, idxB ? idxB + off : nullptr,
                               n, EA, EB, n_layers, dims, packed, out + off, oob, stream);
    };
    // The time of the one-wave-per-tile kernel is a staircase of rounds of 4 x CUs tiles (27.2-28.7 us per round at 128-256-128
    // on an MI355X with layer 1's weights in LDS, 24-25 us for a second round; 29.2-31.4 us streaming them), ncf_score_fused's
    // small-batch kernel one of half rounds (22.4-23.0 us up to 2 x CUs tiles, 31.6-31.8 up to 3 x CUs).
    // So a batch of at most half a round, and a ragged last round of at most half a round, go to ncf_score_fused (its small
    // kernel there); anything more costs a full round of this kernel.  Identity ids (NULL) cannot be offset: no split there.
    const int64_t tiles = (B + 31) / 32;
    const int64_t round = 4 * (int64_t)num_cus();
    const int64_t full = tiles / round, rem = tiles % round;
    int64_t head = B;
    if (rem > 0 && rem * 1000 <= round * NCF_PART_HYBRID_MAX_PERMILLE && (full == 0 || (idxA && idxB))) head = full * round * 32;
    if (head == 0) return plain(0, B);
    const BlobPtrs w = blob_ptrs(packed, dims, n_layers);
    PartialArgs a;
    a.P = (const float*)P; a.rowsA = rowsA; a.ldP = ldP;
    a.tabB = (const float*)tabB; a.rowsB = rowsB; a.ldB = ldB;
    a.idxA = idxA; a.idxB = idxB; a.B = head; a.QA = EA / 8;
    a.Wp1 = w.Wp1; a.Wp2 = w.Wp2; a.b2 = w.b2; a.wl = w.wl; a.bl = w.bl;
    a.out = out; a.oob = oob;
#if NCF_PART_STAMP
    a.stamps = g_stamp_buf;
#endif
    partial_dispatch(EB / 8, N1, n_layers == 3 ? dims[2] : 0, &a, s);
    const int rc = check_launch("ncf_score_fused_partial");
    if (rc != NCF_OK || head == B) return rc;
    return plain(head, B - head);
}
