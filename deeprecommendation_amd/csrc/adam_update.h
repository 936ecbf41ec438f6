// The per-element Adam update shared by ncf_adam_step (backward.hip: every element of a tensor) and ncf_adam_rows
// (adam_rows.hip: the rows a batch touched).  ONE function, so that a row touched exactly once in a step gets the bits the
// dense kernel gives it.
#pragma once
#include "ncf_common.h"
#include <math.h>

namespace ncf {

// Host-side constants of one step (double arithmetic, as torch's single-tensor path): lr / (1 - b1^t), 1 / sqrt(1 - b2^t).
struct AdamCoef {
    float lr_over_bc1, beta1, beta2, inv_sqrt_bc2, eps, wd;
};

inline AdamCoef adam_coef(float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    return AdamCoef{(float)(lr / bc1), beta1, beta2, (float)(1.0 / sqrt(bc2)), eps, weight_decay};
}

//   g += wd * p;  m += (1 - b1) * (g - m);  v = b2 * v + (1 - b2) * g * g;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// — the operation order of torch.optim.Adam's single-tensor path (amsgrad / maximize off).
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamCoef& k) {
    const float gg = k.wd != 0.f ? g + k.wd * p : g;
    m = m + (1.f - k.beta1) * (gg - m);
    v = k.beta2 * v + (1.f - k.beta2) * gg * gg;
    const float denom = sqrtf(v) * k.inv_sqrt_bc2 + k.eps;
    p = p - k.lr_over_bc1 * (m / denom);
}

}  // namespace ncf
