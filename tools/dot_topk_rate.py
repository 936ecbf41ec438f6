"""Dev tool (GPU box, by hand; not part of bench.py): rate of the fused dot-product top-K (ncf_dot_topk) against score-then-select.

For D in {64, 256}, k in {10, 100} and users x items in {512 x 65 536, 4096 x 65 536}: microseconds per call (HIP events over
back-to-back calls) of native.dot_topk over an MF model's tables, of the same ranking through top_k_items(..., fused=False) (scores
block by block through ncf_gather_dot, then ncf_topk_rows), the speed-up, and the fused call's fraction of the fp32 MFMA peak
(157.3 TF) at 2 B I D flop; the streaming copy ceiling (ncf_probe_copy) of the same run is printed alongside.  The two routes'
outputs are checked equal.  Prints one JSON object."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deeprecommendation_amd import native  # noqa: E402
from topk_rate import copy_ceiling, events_us  # noqa: E402

F32_MFMA_PEAK_TF = 157.3


def rates(dev):
    from deeprecommendation_amd.recommend import top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    out = []
    I = 65536
    for D in (64, 256):
        torch.manual_seed(D)
        m = MF(item_dim=I, user_dim=4096, item_emb=D, user_emb=D).to(dev).eval()
        cache = m._refresh()
        ta = m._table("user", m.user_embeddings[0], cache)
        tb = m._table("item", m.item_embeddings[0], cache)
        for B in (512, 4096):
            users = torch.arange(B, device=dev)
            for k in (10, 100):
                fused_us = events_us(lambda: native.dot_topk(ta, users, tb, None, k), 10 if B == 4096 else 30, settle=2)
                unfused_us = events_us(lambda: top_k_items(m, users, k, fused=False), 3, settle=1)
                a = native.dot_topk(ta, users, tb, None, k)
                b = top_k_items(m, users, k, fused=False)
                same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].long(), b[1]) and torch.equal(a[2], b[2]))
                tf = 2.0 * B * I * D / (fused_us * 1e-6) / 1e12
                out.append({"D": D, "users": B, "items": I, "k": k, "fused_us": round(fused_us, 1), "unfused_us": round(unfused_us, 1),
                            "speedup": round(unfused_us / fused_us, 2), "fused_TF": round(tf, 1),
                            "frac_f32_mfma_peak": round(tf / F32_MFMA_PEAK_TF, 3), "bit_equal": same})
    return out


def main():
    dev = torch.device("cuda:0")
    native.load_library()
    res = {"copy_ceiling_GBps": round(copy_ceiling(dev), 1), "dot_topk": rates(dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
