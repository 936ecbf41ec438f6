// Explanations from the logit table: for MANY (user, winner) pairs, the rated items whose attention weight exceeds the user's
// threshold — the `because` / `attention` columns of the reference's web backend (webapp/backend.py:105-121), without the dense
// (pairs x catalogue) weight matrix.  ncf_attn_logits' table ST (attn_cross.hip) holds every logit: a winner's weights are a column
// lookup over its user's rated set, a softmax and a small selection.
//
// One wave = one (user, slot) pair, four pairs per workgroup, no barrier (the waves of a workgroup share nothing).  Lane l owns the
// entries beg + l, beg + l + 64, ... of the user's row in every pass:
//   passes 1-2  the column softmax of attn_table.h: the logits s_e = ST[col_e, c], their maximum m and the denominator l.
//   pass 3  w_e = exp_le0(s_e - m) / l, a function of (s_e, m, l) alone; a valid entry with w_e > thr[u] counts, and its key
//           (topk_map(w_e) << 32 | ~entry index: larger weight first, then the entry stored earlier) is appended to the wave's key
//           buffer; past 192 keys the buffer is cut to the E best (wave_reselect) and the E-th key becomes a floor for later ones.
//   final   at most E keys are left, one per lane; a lane's slot is the number of larger keys (the keys are distinct).
// No atomics; every order is fixed: two calls on the same inputs give the same bits.
#include "attn_table.h"
#include "topk_common.h"

namespace ncf {

constexpr int kExMaxReasons = 64;      // one key per lane in the final ranking
constexpr int kExWaves = 4;
constexpr int kExBuf = 4 * kWave;      // wave_reselect's capacity

__global__ __launch_bounds__(kExWaves* kWave) void attn_explain_kernel(
    const float* __restrict__ st, int64_t ldst, int64_t Ir, int64_t Ic, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const float* __restrict__ val, int64_t n_rows, const int64_t* __restrict__ user_rows,
    const int64_t* __restrict__ items, int64_t pairs, int64_t k, const float* __restrict__ thr, int E, int32_t* __restrict__ rcol,
    float* __restrict__ rw, float* __restrict__ rval, int32_t* __restrict__ rcnt, int32_t* __restrict__ oob) {
    __shared__ unsigned long long bufs[kExWaves][kExBuf];
    __shared__ float caches[kExWaves][kTableCache];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p = (int64_t)blockIdx.x * kExWaves + wave;
    if (p >= pairs) return;                                            // wave-uniform; the kernel has no barrier
    const int64_t u = p / k;
    const int64_t row = user_rows[u], c = items[p];
    const bool row_ok = row >= 0 && row < n_rows, cand_ok = c >= 0 && c < Ic;
    if (oob && lane == 0 && (!row_ok || (!cand_ok && c != -1))) *oob = 1;   // sticky; -1 is an empty slot, not an error
    const bool live = row_ok && cand_ok;
    const int64_t beg = live ? rowptr[row] : 0, end = live ? rowptr[row + 1] : 0;
    const float t = thr[u];
    unsigned long long* buf = bufs[wave];

    // ---------------- passes 1-2: the logits, their exact maximum and the denominator ----------------
    const TableColumn tc{st + (cand_ok ? c : 0), ldst, Ir, col, beg, end, caches[wave], lane};
    const float m = tc.max();
    const bool any = m != -INFINITY;                                   // false: empty / fully masked row, all -inf column, dead pair
    const float l = tc.denominator(m);

    // ---------------- pass 3: weights, the count, the E best keys ----------------
    int cnt = 0, n = 0;
    unsigned long long floor_key = 0ull;
    if (any)
        for (int64_t e0 = beg; e0 < end; e0 += kWave) {
            const int64_t e = e0 + lane;
            bool q = false;
            unsigned long long key = 0ull;
            if (e < end) {
                const int cc = col[e];
                const float w = exp_le0(tc.cached(e0, e) - m) / l;
                q = cc >= 0 && cc < Ir && w > t;                       // a NaN weight never qualifies
                key = ((unsigned long long)topk_map(w) << 32) | (0xFFFFFFFFu - (uint32_t)(e - beg));
            }
            cnt += __popcll(__ballot(q));
            const bool keep = q && key > floor_key;
            const unsigned long long mk = __ballot(keep);
            if (keep) buf[n + lanes_below(mk)] = key;                  // n <= kExBuf - 64 here
            n += __popcll(mk);
            if (n > kExBuf - kWave) {
                wave_lds_sync();
                floor_key = wave_reselect(buf, n, E, lane);
                n = E;
                wave_lds_sync();
            }
        }
    wave_lds_sync();
    if (n > E) {
        wave_reselect(buf, n, E, lane);
        n = E;
        wave_lds_sync();
    }

    // ---------------- final: lane = one kept key; its slot = the number of larger keys ----------------
    const unsigned long long mine = lane < n ? buf[lane] : 0ull;
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += buf[j] > mine ? 1 : 0;
    const int64_t ob = p * E;
    if (lane < n) {
        const int64_t e = beg + (0xFFFFFFFFu - (uint32_t)mine);
        rcol[ob + rank] = col[e];
        rw[ob + rank] = topk_unmap((uint32_t)(mine >> 32));
        rval[ob + rank] = val[e];
    } else if (lane < E) {
        rcol[ob + lane] = -1;
        rw[ob + lane] = 0.f;
        rval[ob + lane] = 0.f;
    }
    if (lane == 0) rcnt[p] = cnt;
}

}  // namespace ncf

using namespace ncf;

extern "C" int ncf_attn_explain_max_reasons(void) { return kExMaxReasons; }

extern "C" int ncf_attn_explain(const float* st, int64_t ldst, int64_t Ir, int64_t Ic, const int64_t* rowptr, const int32_t* col,
                                const float* val, int64_t n_rows, const int64_t* user_rows, int64_t U, const int64_t* items, int64_t k,
                                const float* thr, int max_reasons, int32_t* reason_col, float* reason_w, float* reason_val,
                                int32_t* reason_cnt, int32_t* oob, ncf_stream_t stream) {
    if (max_reasons < 1 || max_reasons > kExMaxReasons)
        return fail(NCF_EUNSUPPORTED, "ncf_attn_explain: max_reasons = %d is outside 1 .. %d", max_reasons, kExMaxReasons);
    if (Ir < 0 || Ic < 0 || n_rows < 0 || U < 0 || k < 0) return fail(NCF_EINVAL, "ncf_attn_explain: bad sizes");
    if (U == 0 || k == 0) return NCF_OK;
    if ((!st && Ir > 0 && Ic > 0) || !rowptr || !user_rows || !items || !thr) return fail(NCF_EINVAL, "ncf_attn_explain: null pointer");
    if (!reason_col || !reason_w || !reason_val || !reason_cnt) return fail(NCF_EINVAL, "ncf_attn_explain: null output pointer");
    if (ldst < Ic) return fail(NCF_EINVAL, "ncf_attn_explain: leading dimension smaller than row");
    if (U > ((int64_t)0x7FFFFFFF * kExWaves) / k)
        return fail(NCF_EUNSUPPORTED, "ncf_attn_explain: more than 2^31 - 1 workgroups");
    const int64_t pairs = U * k;
    const int64_t grid = (pairs + kExWaves - 1) / kExWaves;
    hipLaunchKernelGGL(attn_explain_kernel, dim3((unsigned)grid), dim3(kExWaves * kWave), 0, (hipStream_t)stream, st, ldst, Ir, Ic,
                       rowptr, col, val, n_rows, user_rows, items, pairs, k, thr, max_reasons, reason_col, reason_w, reason_val,
                       reason_cnt, oob);
    return check_launch("ncf_attn_explain");
}
