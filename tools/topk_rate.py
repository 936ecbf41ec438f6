"""Dev tool (GPU box, by hand; not part of bench.py): rate of ncf_topk_rows and cost of recommend_for_user.

1. top-K over rows x cols in {1 x 65 536, 1 x 1 048 576, 512 x 65 536, 4096 x 3 706} at k in {10, 100, 1000}: microseconds per call
   (HIP events over back-to-back calls) and GB/s of score bytes read, next to the chip's streaming copy ceiling measured in the same
   run (ncf_probe_copy, read + written bytes).
2. recommend_for_user at config-3 sizes (65 536-item catalogue, F = 2094, 256 rated items, k = 10): milliseconds per request end to
   end (host work and the k-row copies included) next to the catalogue forward alone (the same SparseRatings call the function
   makes first), with the catalogue tensor repeated request after request.
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402


def events_us(fn, reps, settle=5):
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def copy_ceiling(dev, nbytes=1 << 30):
    lib = native.load_library()
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream(dev).cuda_stream
    us = events_us(lambda: native._check(lib.ncf_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes, st)), 20)
    return 2 * nbytes / (us * 1e-6) / 1e9


def topk_rates(dev):
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    for rows, cols in ((1, 65536), (1, 1 << 20), (512, 65536), (4096, 3706)):
        x = torch.randn(rows, cols, device=dev, generator=g)
        for k in (10, 100, 1000):
            us = events_us(lambda: native.topk_rows(x, k), 50)
            out.append({"rows": rows, "cols": cols, "k": k, "us": round(us, 2), "GBps": round(rows * cols * 4 / (us * 1e-6) / 1e9, 1)})
    return out


def recommend_cfg3(dev):
    import pandas as pd
    from deeprecommendation_amd.recommend import recommend_for_user
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF, SparseRatings
    I, F, NNZ, K = 65536, 2094, 256, 10
    rng = np.random.default_rng(0)
    feats = (rng.random((I, F), dtype=np.float32) < 0.02).astype(np.float32)
    cat = pd.DataFrame(feats, index=[f"tt{i:07d}" for i in range(I)])
    torch.manual_seed(0)
    model = AttentionNCF(item_dim=F, item_emb=64, user_emb=64, att_dense=128, mlp_dense_layers=[256, 128]).to(dev).eval()
    users = []
    for s in range(8):
        r = np.random.default_rng(100 + s)
        users.append(pd.Series(index=r.choice(cat.index.to_numpy(), NNZ, replace=False), data=r.integers(1, 11, NNZ) * 0.5, dtype=float))

    def wall_ms(fn, n):
        for j in range(3):
            fn(j)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for j in range(n):
            fn(j)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n

    rec_ms = wall_ms(lambda j: recommend_for_user(model, cat, users[j % 8], k=K), 20)
    from deeprecommendation_amd.recommend import _catalogue
    cat_t, ids = _catalogue(cat, dev)
    # the forward alone, on the same inputs the function builds (rated rows gathered, one CSR row shared by every candidate)
    fwd_inputs = []
    for u in users:
        rated_ids = np.sort(np.unique(u.index))
        pos = torch.from_numpy(ids.get_indexer(rated_ids).astype(np.int64)).to(dev)
        c = (u.loc[rated_ids].values - (u.mean() + 2.5) / 2).astype(np.float32)
        nz = np.nonzero(c != 0)[0]
        fwd_inputs.append((cat_t.index_select(0, pos), SparseRatings(
            torch.tensor([0, len(nz)], device=dev), torch.from_numpy(nz.astype(np.int32)).to(dev), torch.from_numpy(c[nz]).to(dev),
            len(rated_ids), pair_row=torch.zeros(I, dtype=torch.int64, device=dev))))
    with torch.no_grad():
        fwd_ms = wall_ms(lambda j: model(cat_t, *fwd_inputs[j % 8]), 20)
        fwd_dev_us = events_us(lambda: model(cat_t, *fwd_inputs[0]), 20)
        scores = model(cat_t, *fwd_inputs[0]).view(1, I)
        topk_us = events_us(lambda: native.topk_rows(scores, K), 50)
    return {"catalogue": I, "features": F, "rated": NNZ, "k": K, "recommend_ms_per_request": round(rec_ms, 3),
            "forward_alone_ms_wall": round(fwd_ms, 3), "forward_alone_us_events": round(fwd_dev_us, 1),
            "topk_us": round(topk_us, 2), "added_over_forward": round(rec_ms / fwd_ms - 1.0, 3)}


def main():
    dev = torch.device("cuda:0")
    native.load_library()
    res = {"copy_ceiling_GBps": round(copy_ceiling(dev), 1), "topk": topk_rates(dev)}
    for r in res["topk"]:
        r["frac_of_copy_ceiling"] = round(r["GBps"] / res["copy_ceiling_GBps"], 3)
    res["recommend_cfg3"] = recommend_cfg3(dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
