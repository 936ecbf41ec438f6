"""Dev tool (GPU box, by hand; not part of bench.py): rate of the fused MLP top-K (ncf_mlp_topk) against score-then-select.

A BasicNCF with MLP [256, 128] at cfg-2 widths (E = 64 + 64) and at E = 128 + 128; users x items in {512 x 65 536, 4096 x 65 536};
k in {10, 100}: microseconds per call (HIP events over back-to-back calls) of top_k_items through the fused kernel (the default
route) and of top_k_items(..., fused=False) (pair id columns, ncf_score_fused over every pair, ncf_topk_rows), the speed-up, and the
fused call's fraction of the fp32 MFMA peak (157.3 TF) on EXECUTED flop: the per-pair work 2 (EB N1 + N1 N2 + N2) (98 560 at cfg-2
widths) plus the prefix pass's 2 EA N1 per user.  The two routes' outputs are checked equal.  Prints one JSON object."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deeprecommendation_amd import native  # noqa: E402
from topk_rate import events_us  # noqa: E402

F32_MFMA_PEAK_TF = 157.3


def rates(dev):
    from deeprecommendation_amd.recommend import top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    out = []
    I, N1, N2 = 65536, 256, 128
    for E in (64, 128):
        torch.manual_seed(E)
        m = BasicNCF(item_dim=I, user_dim=4096, item_emb=E, user_emb=E, mlp_dense_layers=[N1, N2]).to(dev).eval()
        for B in (512, 4096):
            users = torch.arange(B, device=dev)
            for k in (10, 100):
                fused_us = events_us(lambda: top_k_items(m, users, k), 10 if B == 4096 else 30, settle=2)
                unfused_us = events_us(lambda: top_k_items(m, users, k, fused=False), 3, settle=1)
                a = top_k_items(m, users, k)
                b = top_k_items(m, users, k, fused=False)
                same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                       y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
                flop = 2.0 * B * I * (E * N1 + N1 * N2 + N2) + 2.0 * B * E * N1
                tf = flop / (fused_us * 1e-6) / 1e12
                out.append({"E": f"{E}+{E}", "users": B, "items": I, "k": k, "fused_us": round(fused_us, 1),
                            "unfused_us": round(unfused_us, 1), "speedup": round(unfused_us / fused_us, 2),
                            "flop_per_pair": 2 * (E * N1 + N1 * N2 + N2), "fused_TF": round(tf, 1),
                            "frac_f32_mfma_peak": round(tf / F32_MFMA_PEAK_TF, 3), "bit_equal": same})
    return out


def main():
    dev = torch.device("cuda:0")
    native.load_library()
    print(json.dumps({"mlp_topk": rates(dev)}))


if __name__ == "__main__":
    main()
