/* CPU restatement, in plain C, of the ARITHMETIC ORDER of the fused gather -> MLP kernel
 * (deeprecommendation_amd/csrc/mlp_fused.hip) — TEST INFRASTRUCTURE ONLY (see oracle/ncf_oracle.py for the
 * reference-level oracle this is itself checked against).
 *
 * What it restates: models/basic_ncf.py:37-42 of the reference in table form (Linear(onehot(i)) == W[:, i] + b, then
 * cat(user, item) -> util.py:5-18 MLP with ReLU between layers and a 1-wide last layer), evaluated with exactly the
 * floating-point operation order of the GPU kernel, so that the GPU result can be compared BIT FOR BIT:
 *   - v_mfma_f32_32x32x2_f32 is an exact k-ordered fmaf chain (one rounding per product, MI355X guide), k = lane
 *     half 0 first, then lane half 1; the kernel feeds k = 8q + j (half 0) and k = 8q + 4 + j (half 1) for j = 0..3;
 *   - accumulators start from the bias;
 *   - the last layer is an fmaf chain per lane half over n = 32nt + 8g + 4h + j (nt, g, j ascending), the two halves
 *     are added (half 0 + half 1), then the output bias.
 * Compile without FMA contraction and without fast-math: the only fused operations are the explicit fmaf() calls.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static inline float relu(float x) { return x > 0.f ? x : 0.f; }

/* one layer in MFMA order: out[n] = chain over q, j of (k = 8q+j, then k = 8q+4+j), starting from bias[n] */
static void layer_mfma_order(const float* x, int K, const float* W, const float* b, int N, float* out) {
    for (int n = 0; n < N; ++n) {
        float acc = b[n];
        const float* w = W + (size_t)n * K;
        for (int q = 0; q < K / 8; ++q)
            for (int j = 0; j < 4; ++j) {
                acc = fmaf(w[8 * q + j], x[8 * q + j], acc);
                acc = fmaf(w[8 * q + 4 + j], x[8 * q + 4 + j], acc);
            }
        out[n] = acc;
    }
}

/* N2 == 0: single hidden layer.  Returns 0, or -1 on a shape the kernel does not take either. */
int oracle_score_fused_f32(const float* tabA, int64_t ldA, const float* tabB, int64_t ldB,
                           const int64_t* idxA, const int64_t* idxB, int64_t B, int EA, int EB,
                           const float* W1, const float* b1, int N1,
                           const float* W2, const float* b2, int N2,
                           const float* wl, const float* bl, float* out) {
    const int K0 = EA + EB;
    if (K0 % 8 || N1 % 32 || N2 % 32) return -1;
    const int NL = N2 > 0 ? N2 : N1;
#pragma omp parallel
    {
        float* x = (float*)malloc(sizeof(float) * (size_t)(K0 + N1 + (N2 > 0 ? N2 : 1)));
        float* h1 = x + K0;
        float* h2 = h1 + N1;
#pragma omp for
        for (int64_t p = 0; p < B; ++p) {
            const float* ra = tabA + idxA[p] * ldA;
            const float* rb = tabB + idxB[p] * ldB;
            for (int e = 0; e < EA; ++e) x[e] = ra[e];
            for (int e = 0; e < EB; ++e) x[EA + e] = rb[e];
            layer_mfma_order(x, K0, W1, b1, N1, h1);
            const float* last = h1;
            if (N2 > 0) {
                for (int n = 0; n < N1; ++n) h1[n] = relu(h1[n]);
                layer_mfma_order(h1, N1, W2, b2, N2, h2);
                last = h2;
            }
            float part[2] = {0.f, 0.f};
            for (int h = 0; h < 2; ++h)
                for (int nt = 0; nt < NL / 32; ++nt)
                    for (int g = 0; g < 4; ++g)
                        for (int j = 0; j < 4; ++j) {
                            const int n = 32 * nt + 8 * g + 4 * h + j;
                            part[h] = fmaf(wl[n], relu(last[n]), part[h]);
                        }
            out[p] = (part[0] + part[1]) + bl[0];
        }
        free(x);
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * The extended restatement: the root reference of the fp32 scorer family (ncf_score_fused, ncf_score_folded,
 * ncf_layer1_partial / ncf_score_fused_partial).  On top of the chain order above it restates
 *   - the RANGE RULE of the kernels: ok = 0 <= i < rows; an out-of-range id reads row 0 and every gathered value is multiplied
 *     by the factor (1.0f or 0.0f) at use.  The multiply is a real one: inf * 0 and nan * 0 are NaN, a negative value times 0
 *     is -0.0, as on the device.  *oob is set when any id was out of range;
 *   - identity ids: idx NULL means pair p reads row p (and is out of range from p = rows on);
 *   - the single-table form: EB = 0, tabB unused;
 *   - a NULL bias of any layer, which reads as zeros.
 * ReLU is x > 0 ? x : 0 (a NaN becomes 0, as v_max_f32 gives it).
 */
static inline const float* row_of(const float* tab, int64_t rows, int64_t ld, const int64_t* idx, int64_t p, float* z) {
    const int64_t i = idx ? idx[p] : p;
    const int ok = i >= 0 && i < rows;
    *z = ok ? 1.0f : 0.0f;
    return tab + (ok ? i : 0) * ld;
}

/* the chain of layer_mfma_order over k-groups q0 .. q1-1, continued from acc[] in place; x holds the K inputs */
static void chain_groups(const float* x, int K, const float* W, int N, int q0, int q1, float* acc) {
    for (int n = 0; n < N; ++n) {
        float a = acc[n];
        const float* w = W + (size_t)n * K;
        for (int q = q0; q < q1; ++q)
            for (int j = 0; j < 4; ++j) {
                a = fmaf(w[8 * q + j], x[8 * q + j], a);
                a = fmaf(w[8 * q + 4 + j], x[8 * q + 4 + j], a);
            }
        acc[n] = a;
    }
}

/* the 1-wide layer: per lane half over nt, g, j; half 0 + half 1; then the bias */
static float last_layer(const float* act, int NL, const float* wl, const float* bl) {
    float part[2] = {0.f, 0.f};
    for (int h = 0; h < 2; ++h)
        for (int nt = 0; nt < NL / 32; ++nt)
            for (int g = 0; g < 4; ++g)
                for (int j = 0; j < 4; ++j) {
                    const int n = 32 * nt + 8 * g + 4 * h + j;
                    part[h] = fmaf(wl[n], relu(act[n]), part[h]);
                }
    return (part[0] + part[1]) + (bl ? bl[0] : 0.f);
}

/* ReLU of h1 in place, layer 2 from b2 (NULL: zeros), the 1-wide layer; N2 == 0: the 1-wide layer on h1 */
static float tail_from_h1(float* h1, int N1, const float* W2, const float* b2, int N2, float* h2, const float* wl, const float* bl) {
    if (N2 == 0) return last_layer(h1, N1, wl, bl);
    for (int n = 0; n < N1; ++n) h1[n] = relu(h1[n]);
    for (int n = 0; n < N2; ++n) h2[n] = b2 ? b2[n] : 0.f;
    chain_groups(h1, N1, W2, N2, 0, N1 / 8, h2);
    return last_layer(h2, N2, wl, bl);
}

int oracle_score_fused_f32_ex(const float* tabA, int64_t rowsA, int64_t ldA, const float* tabB, int64_t rowsB, int64_t ldB,
                              const int64_t* idxA, const int64_t* idxB, int64_t B, int EA, int EB,
                              const float* W1, const float* b1, int N1, const float* W2, const float* b2, int N2,
                              const float* wl, const float* bl, float* out, int* oob) {
    const int K0 = EA + EB;
    if (EA <= 0 || EB < 0 || EA % 8 || EB % 8 || N1 % 32 || N2 % 32 || !tabA || (EB > 0 && !tabB)) return -1;
    int any = 0;
#pragma omp parallel reduction(| : any)
    {
        float* x = (float*)malloc(sizeof(float) * (size_t)(K0 + N1 + (N2 > 0 ? N2 : 1)));
        float* h1 = x + K0;
        float* h2 = h1 + N1;
#pragma omp for
        for (int64_t p = 0; p < B; ++p) {
            float zA, zB = 1.0f;
            const float* ra = row_of(tabA, rowsA, ldA, idxA, p, &zA);
            for (int e = 0; e < EA; ++e) x[e] = ra[e] * zA;
            if (EB > 0) {
                const float* rb = row_of(tabB, rowsB, ldB, idxB, p, &zB);
                for (int e = 0; e < EB; ++e) x[EA + e] = rb[e] * zB;
            }
            any |= (zA == 0.0f) | (zB == 0.0f);
            for (int n = 0; n < N1; ++n) h1[n] = b1 ? b1[n] : 0.f;
            chain_groups(x, K0, W1, N1, 0, K0 / 8, h1);
            out[p] = tail_from_h1(h1, N1, W2, b2, N2, h2, wl, bl);
        }
        free(x);
    }
    if (oob) *oob = any;
    return 0;
}

/* P[rowsA + 1][N1] of ncf_layer1_partial: layer 1's chain from b1 truncated after table A's EA / 8 groups, for every row of A and
 * (last row) for an out-of-range id: row 0 times 0.0f.  W1 is [N1][K0]. */
int oracle_layer1_partial_f32(const float* tabA, int64_t rowsA, int64_t ldA, int EA, int K0, const float* W1, const float* b1,
                              int N1, float* P) {
    if (EA <= 0 || EA % 8 || K0 % 8 || EA > K0 || N1 % 32 || rowsA < 1) return -1;
    float* x = (float*)malloc(sizeof(float) * (size_t)K0);
    for (int64_t r = 0; r <= rowsA; ++r) {
        const float z = r < rowsA ? 1.0f : 0.0f;
        const float* ra = tabA + (r < rowsA ? r : 0) * ldA;
        for (int e = 0; e < K0; ++e) x[e] = e < EA ? ra[e] * z : 0.f;
        float* acc = P + (size_t)r * N1;
        for (int n = 0; n < N1; ++n) acc[n] = b1 ? b1[n] : 0.f;
        chain_groups(x, K0, W1, N1, 0, EA / 8, acc);
    }
    free(x);
    return 0;
}

/* ncf_score_folded: s = PA_row * zA + PB_row * zB (both products exact, one rounding in the sum), ReLU, layer 2 as the same chain
 * from b2, the same 1-wide layer.  b1 lives in PA: an out-of-range A id drops it with the row. */
int oracle_score_folded_f32(const float* PA, int64_t rowsA, int64_t ldA, const float* PB, int64_t rowsB, int64_t ldB,
                            const int64_t* idxA, const int64_t* idxB, int64_t B, int N1,
                            const float* W2, const float* b2, int N2, const float* wl, const float* bl, float* out, int* oob) {
    if (N1 % 32 || N2 % 32 || N2 <= 0 || !PA || !PB) return -1;
    int any = 0;
#pragma omp parallel reduction(| : any)
    {
        float* h1 = (float*)malloc(sizeof(float) * (size_t)(N1 + N2));
        float* h2 = h1 + N1;
#pragma omp for
        for (int64_t p = 0; p < B; ++p) {
            float zA, zB;
            const float* ra = row_of(PA, rowsA, ldA, idxA, p, &zA);
            const float* rb = row_of(PB, rowsB, ldB, idxB, p, &zB);
            any |= (zA == 0.0f) | (zB == 0.0f);
            for (int n = 0; n < N1; ++n) {
                const float a = ra[n] * zA, b = rb[n] * zB;
                h1[n] = a + b;
            }
            out[p] = tail_from_h1(h1, N1, W2, b2, N2, h2, wl, bl);
        }
        free(h1);
    }
    if (oob) *oob = any;
    return 0;
}
