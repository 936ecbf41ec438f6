// SLIM (Ning & Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender Systems"), the sparse item-item baseline EASE is
// measured against, on gfx950: column j of W minimises
//     1/2 w^T G w - G[j]^T w + 1/2 l2 |w|^2 + l1 |w|_1,   w[j] = 0   (and w >= 0 when `positive`),     G = X^T X (ncf_ease_gram),
// by cyclic coordinate descent on the Gram matrix.  W is served by ncf_ease_scores / ncf_ease_predict as EASE's weights are.
//
// THE CONTRACT (restated from include/ncf_abi.h).  State of one column: w (I) and q = G w (I), both +0.0f at a cold start, and
// d[k] = G[k][k].  One sweep visits k = 0 .. I - 1 in ascending order and skips k == j:
//     t = d[k] * w[k];  r = q[k] - t;  rho = G[j][k] - r;  den = d[k] + l2
//     positive:  a = rho - l1;  wn = (a > 0 && den > 0) ? a / den : +0.0f
//     signed:    rho >  l1 && den > 0 -> (rho - l1) / den;   rho < -l1 && den > 0 -> (rho + l1) / den;   else +0.0f
//     delta = wn - w[k]
//     if delta != 0:  for every i: q[i] = q[i] + delta * G[k][i];  w[k] = wn;  steps += 1
// every product, sum and quotient rounded on its own (THIS FILE IS BUILT WITH -ffp-contract=off, build.py EXTRA_FLAGS, and no
// fast-math flag may be added to it; hipcc's default fp32 division is the correctly rounded one and is relied on).  A column stops
// after the first sweep whose largest |delta| is <= tol, or after max_sweeps.  Warm start: w is the output row with w[j] = +0.0f,
// and q = +0; for k ascending with w[k] != 0: q = q + w[k] * G[k].  No reduction over floats occurs anywhere, so the result is one
// fixed function of its inputs (tests/slim_ref.py, bit for bit, `sweeps` and `steps` included), whatever the workgroup size.
//
// HOW THE SERIAL LOOP RUNS IN PARALLEL.  While q does not change, the candidate updates of a block of coordinates can be evaluated
// side by side, and the first coordinate of the block with delta != 0 is the one the serial loop would have updated first: every
// coordinate before it left q untouched.  One workgroup of T threads owns a column and repeats
//     screen:   thread t evaluates coordinate k0 + t of the block [k0, k0 + T) that is not behind the last update; a wave ballot and
//               a minimum over the waves (slim_first: one barrier) name the first coordinate with delta != 0
//     apply:    if there is one, every thread runs its share of the axpy q += delta * G[k] (row k of G, coalesced) and the owner of k
//               stores w[k]; screening resumes behind k
//     advance:  otherwise k0 += T
// With an L1 penalty most coordinates never move: a sweep costs about I / T screens plus one axpy per moving coordinate.
//
// WHO OWNS WHAT.  k0 is a multiple of T, so thread t is the only thread that ever reads or writes q[i] and w[i] for i = t (mod T):
// the zeroing, the screen of coordinate i and the axpy's element i are all thread t's.  q (in LDS) and w (the output row, in global
// memory) therefore need no ordering between threads; the only barrier of the loop is the one inside slim_first.  d[k] is read from
// G's diagonal (the entry takes no workspace): one load per screened coordinate, beside the coalesced loads of G[j][k] and w[k].
//
// A column that the list names again is not solved again (two workgroups would write one row of Wt while reading it): the later
// listing stores -(first listing + 1) in its `sweeps` slot and slim_dup_kernel, launched behind the solve, copies the first
// listing's three outputs into it.
#include "ncf_common.h"

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

#define NCF_SLIM_SMALL_THREADS 256        // workgroup of a catalogue of at most NCF_SLIM_SMALL_ITEMS items
#define NCF_SLIM_SMALL_ITEMS 2048
#define NCF_SLIM_THREADS 1024
#define NCF_SLIM_SLOT_BYTES 512           // LDS in front of q: the slots of slim_first, [2][T / 64] of (k, wn, delta), and one word

namespace ncf {

struct SlimPick {
    int k;                                // INT_MAX: no coordinate of the block qualifies
    float wn, delta;
};

// The lowest k among the threads with `pred`, and that thread's wn and delta, the same in every thread.  sk / sw / sd: [2][T / 64]
// in LDS; consecutive calls alternate `par`, so a call's slots are not written again before every thread has passed the next call's
// barrier.  Every thread of the workgroup must call it.
template <int T>
__device__ __forceinline__ SlimPick slim_first(bool pred, int k, float wn, float delta, int (*sk)[T / 64], float (*sw)[T / 64],
                                               float (*sd)[T / 64], int par) {
    constexpr int NW = T / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pred);
    if (m == 0ull) {
        if (lane == 0) sk[par][wave] = INT_MAX;
    } else if (lane == __ffsll(m) - 1) {
        sk[par][wave] = k;
        sw[par][wave] = wn;
        sd[par][wave] = delta;
    }
    __syncthreads();
    SlimPick p;
    p.k = INT_MAX;
    p.wn = p.delta = 0.0f;
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {                      // waves hold ascending coordinates: the lowest wave with a hit wins
        const int kk = sk[par][w];
        if (kk != INT_MAX) {
            p.k = kk;
            p.wn = sw[par][w];
            p.delta = sd[par][w];
        }
    }
    return p;
}

// q[i] = q[i] + a * g[i] for this thread's elements i = t (mod T)
template <int T>
__device__ __forceinline__ void slim_axpy(float* q, const float* __restrict__ g, float a, int I) {
#pragma unroll 4
    for (int i = threadIdx.x; i < I; i += T) {
        const float p = a * g[i];
        q[i] = q[i] + p;
    }
}

// One workgroup per listed column: blockIdx.x = c.
template <int T>
__global__ __launch_bounds__(T) void slim_solve_kernel(const float* __restrict__ G, int I, int64_t ldg, const int32_t* __restrict__ cols,
                                                       float l1, float l2, int positive, int warm, int max_sweeps, float tol, float* Wt,
                                                       int64_t ldw, int32_t* __restrict__ sweeps, int32_t* __restrict__ steps,
                                                       float* __restrict__ last, int32_t* oob) {
    // all of the LDS is dynamic (a kernel with static LDS cannot have its dynamic limit raised to the whole 160 KiB): the slots of
    // slim_first and one word in the first NCF_SLIM_SLOT_BYTES, then q
    extern __shared__ __align__(16) unsigned char slim_lds[];
    constexpr int NW = T / 64;
    int (*sk)[NW] = reinterpret_cast<int (*)[NW]>(slim_lds);
    float (*sw)[NW] = reinterpret_cast<float (*)[NW]>(slim_lds + 8 * NW);
    float (*sd)[NW] = reinterpret_cast<float (*)[NW]>(slim_lds + 16 * NW);
    int& sfirst = *reinterpret_cast<int*>(slim_lds + 24 * NW);
    static_assert(24 * NW + 4 <= NCF_SLIM_SLOT_BYTES, "the slots fit their share of the LDS");
    float* q = reinterpret_cast<float*>(slim_lds + NCF_SLIM_SLOT_BYTES);           // [I]
    const int c = blockIdx.x, tid = threadIdx.x;
    const int j = cols[c];
    if (j < 0 || j >= I) {                                   // uniform: nothing is read or written through this column
        if (tid == 0) {
            if (oob) atomicOr(oob, 1);
            sweeps[c] = 0;
            steps[c] = 0;
            last[c] = 0.0f;
        }
        return;
    }
    int first = INT_MAX;                                     // the first listing of this column before c, if any
    for (int e = tid; e < c; e += T)
        if (cols[e] == j) {
            first = e;
            break;
        }
    if (tid == 0) sfirst = INT_MAX;
    __syncthreads();
    if (first != INT_MAX) atomicMin(&sfirst, first);
    __syncthreads();
    first = sfirst;
    if (first != INT_MAX) {                                  // uniform
        if (tid == 0) sweeps[c] = -(first + 1);
        return;
    }
    float* wrow = Wt + (int64_t)j * ldw;
    const float* __restrict__ gj = G + (int64_t)j * ldg;
    for (int i = tid; i < I; i += T) {
        q[i] = 0.0f;
        if (!warm || i == j) wrow[i] = 0.0f;
    }
    int par = 0;
    if (warm) {
        for (int k0 = 0; k0 < I; k0 += T) {
            const int k = k0 + tid;
            const float wk = k < I ? wrow[k] : 0.0f;
            int from = k0;
            for (;;) {
                const SlimPick p = slim_first<T>(k >= from && wk != 0.0f, k, wk, 0.0f, sk, sw, sd, par);
                par ^= 1;
                if (p.k == INT_MAX) break;
                slim_axpy<T>(q, G + (int64_t)p.k * ldg, p.wn, I);
                from = p.k + 1;
            }
        }
    }
    int nsweeps = 0, nsteps = 0;
    float maxd;
    do {
        maxd = 0.0f;
        for (int k0 = 0; k0 < I; k0 += T) {
            const int k = k0 + tid;
            const bool mine = k < I && k != j;
            float dk = 0.0f, gjk = 0.0f, wk = 0.0f;
            if (mine) {
                dk = G[(int64_t)k * ldg + k];
                gjk = gj[k];
                wk = wrow[k];
            }
            const float den = dk + l2;
            int from = k0;
            for (;;) {
                float wn = 0.0f, delta = 0.0f;
                if (mine && k >= from) {
                    const float t = dk * wk;
                    const float r = q[k] - t;
                    const float rho = gjk - r;
                    if (positive) {
                        const float a = rho - l1;
                        if (a > 0.0f && den > 0.0f) wn = a / den;
                    } else if (rho > l1 && den > 0.0f) {
                        wn = (rho - l1) / den;
                    } else if (rho < -l1 && den > 0.0f) {
                        wn = (rho + l1) / den;
                    }
                    delta = wn - wk;
                }
                const SlimPick p = slim_first<T>(delta != 0.0f, k, wn, delta, sk, sw, sd, par);
                par ^= 1;
                if (p.k == INT_MAX) break;
                slim_axpy<T>(q, G + (int64_t)p.k * ldg, p.delta, I);
                if (p.k == k) wrow[k] = p.wn;                // behind `from` from now on: wk is not read again in this sweep
                ++nsteps;
                const float ad = fabsf(p.delta);
                if (ad > maxd) maxd = ad;
                from = p.k + 1;
            }
        }
        ++nsweeps;
    } while (!(maxd <= tol) && nsweeps < max_sweeps);
    if (tid == 0) {
        sweeps[c] = nsweeps;
        steps[c] = nsteps;
        last[c] = maxd;
    }
}

// A later listing of a column takes the outputs of the first one (which is no later listing itself, so nothing here is read while
// it is written).
__global__ __launch_bounds__(256) void slim_dup_kernel(int64_t n, int32_t* sweeps, int32_t* steps, float* last) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int32_t s = sweeps[c];
    if (s >= 0) return;
    const int64_t f = -(int64_t)s - 1;
    sweeps[c] = sweeps[f];
    steps[c] = steps[f];
    last[c] = last[f];
}

template <int T>
static int slim_launch(const char* who, const float* G, int64_t I, int64_t ldg, const int32_t* cols, int64_t n, float l1, float l2,
                       int positive, int warm, int max_sweeps, float tol, float* Wt, int64_t ldw, int32_t* sweeps, int32_t* steps,
                       float* last, int32_t* oob, hipStream_t s) {
    const size_t lds = NCF_SLIM_SLOT_BYTES + sizeof(float) * (size_t)I;
    static std::atomic<unsigned long long> done{0};
    if (lds > 64 * 1024 && !raise_lds((const void*)slim_solve_kernel<T>, done))
        return fail(NCF_EUNSUPPORTED, "%s: cannot reserve %zu bytes of LDS", who, lds);
    hipLaunchKernelGGL(slim_solve_kernel<T>, dim3((unsigned)n), dim3(T), lds, s, G, (int)I, ldg, cols, l1, l2, positive, warm, max_sweeps,
                       tol, Wt, ldw, sweeps, steps, last, oob);
    hipLaunchKernelGGL(slim_dup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, sweeps, steps, last);
    return check_launch(who);
}

}  // namespace ncf

using namespace ncf;

static_assert(sizeof(float) * NCF_SLIM_MAX_ITEMS + NCF_SLIM_SLOT_BYTES <= 160 * 1024, "q and the slots share the 160 KiB of LDS");

extern "C" int ncf_slim_solve(const float* G, int64_t I, int64_t ldg, const int32_t* cols, int64_t n, float l1, float l2, int positive,
                              int warm, int max_sweeps, float tol, float* Wt, int64_t ldw, int32_t* sweeps, int32_t* steps, float* last,
                              int32_t* dev_oob_flag, ncf_stream_t stream) {
    const char* who = "ncf_slim_solve";
    if (I < 0 || n < 0) return fail(NCF_EINVAL, "%s: negative size I=%lld n=%lld", who, (long long)I, (long long)n);
    if (ldg < I) return fail(NCF_EINVAL, "%s: ldg = %lld < I = %lld", who, (long long)ldg, (long long)I);
    if (ldw < I) return fail(NCF_EINVAL, "%s: ldw = %lld < I = %lld", who, (long long)ldw, (long long)I);
    if (!isfinite(l1) || l1 < 0.f || !isfinite(l2) || l2 < 0.f) return fail(NCF_EINVAL, "%s: l1 and l2 must be finite and >= 0", who);
    if (!isfinite(tol) || tol < 0.f) return fail(NCF_EINVAL, "%s: tol must be finite and >= 0", who);
    if (max_sweeps < 1) return fail(NCF_EINVAL, "%s: max_sweeps = %d (at least 1)", who, max_sweeps);
    if (!aligned(G, 4) || !aligned(cols, 4) || !aligned(Wt, 4) || !aligned(sweeps, 4) || !aligned(steps, 4) || !aligned(last, 4) ||
        !aligned(dev_oob_flag, 4))
        return fail(NCF_EINVAL, "%s: a misaligned array", who);
    if (I > NCF_SLIM_MAX_ITEMS) return fail(NCF_EUNSUPPORTED, "%s: I = %lld items (at most %d)", who, (long long)I, NCF_SLIM_MAX_ITEMS);
    if (n > 0x7ffffffe) return fail(NCF_EUNSUPPORTED, "%s: %lld columns in one call", who, (long long)n);
    if (n == 0) return NCF_OK;
    if (!cols || !sweeps || !steps || !last) return fail(NCF_EINVAL, "%s: null column list or per-column output", who);
    if (I > 0 && (!G || !Wt)) return fail(NCF_EINVAL, "%s: null G or Wt", who);
    hipStream_t s = (hipStream_t)stream;
    if (I <= NCF_SLIM_SMALL_ITEMS)
        return slim_launch<NCF_SLIM_SMALL_THREADS>(who, G, I, ldg, cols, n, l1, l2, positive != 0, warm != 0, max_sweeps, tol, Wt, ldw, sweeps,
                                                   steps, last, dev_oob_flag, s);
    return slim_launch<NCF_SLIM_THREADS>(who, G, I, ldg, cols, n, l1, l2, positive != 0, warm != 0, max_sweeps, tol, Wt, ldw, sweeps, steps,
                                         last, dev_oob_flag, s);
}
