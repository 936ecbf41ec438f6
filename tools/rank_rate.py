"""Dev tool (GPU box, by hand; not part of bench.py): rate of the exact-rank kernels (ncf_dot_rank, ncf_mlp_rank) beside the top-K
kernels of the same build.

    python tools/rank_rate.py dot [--repeats 3]      python tools/rank_rate.py mlp [--repeats 3]

dot: an MF model at D in {64, 256}, users x items in {512 x 65 536, 4096 x 65 536}: native.dot_rank at max_targets 1 / 20 / the cap
     (every user with that many targets), native.dot_topk at k = 10 and k = 100, and the unfused route (rank_of_items(fused=False):
     scores block by block through ncf_gather_dot, then ncf_rank_rows, max_targets = 1).
mlp: a BasicNCF with MLP [256, 128] at E = 64 + 64 and 128 + 128, same shapes: native.mlp_rank at max_targets 1 / 20 against
     native.mlp_topk at k = 10.
The calls being compared are interleaved inside one run: each repeat times every call once (HIP events over back-to-back calls after
a warm-up), and the result is the range (min .. max) of microseconds per call over the repeats, with the fraction of the fp32 MFMA
peak (157.3 TF; dot: 2 B I D flop, mlp: executed flop as tools/mlp_topk_rate.py counts them) at the median.  The fused ranks are
checked equal to the unfused route's.  Every shape runs in a child process of its own under a time limit, and a child that fails
ends the run.  Prints one JSON object per shape."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

F32_MFMA_PEAK_TF = 157.3
I = 65536


def _targets(B, n, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    col = torch.randint(0, I, (B * n,), device=dev, generator=g).to(torch.int32)
    return torch.arange(0, B * n + 1, n, dtype=torch.int64, device=dev), col


def _interleaved(calls, repeats, reps):
    from topk_rate import events_us
    for fn in calls.values():
        fn()                                            # every shape warmed before any timing
    torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            us[name].append(events_us(fn, reps.get(name, reps["*"]), settle=1))
    return us


def _summary(us, flop):
    out = {}
    for name, v in us.items():
        med = statistics.median(v)
        out[name] = {"us_min": round(min(v), 1), "us_max": round(max(v), 1), "us_median": round(med, 1),
                     "frac_f32_mfma_peak": round(flop / (med * 1e-6) / 1e12 / F32_MFMA_PEAK_TF, 3)}
    return out


def dot_shape(D, B, repeats):
    from deeprecommendation_amd import native, rank_of_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    dev = torch.device("cuda:0")
    torch.manual_seed(D)
    m = MF(item_dim=I, user_dim=4096, item_emb=D, user_emb=D).to(dev).eval()
    cache = m._refresh()
    ta = m._table("user", m.user_embeddings[0], cache)
    tb = m._table("item", m.item_embeddings[0], cache)
    users = torch.arange(B, device=dev)
    cap = native.RANK_MAX_TARGETS
    tg = {n: _targets(B, n, dev) for n in (1, 20, cap)}
    calls = {"dot_topk_k10": lambda: native.dot_topk(ta, users, tb, None, 10),
             "dot_rank_mt1": lambda: native.dot_rank(ta, users, tb, None, tg[1], 1),
             "dot_topk_k100": lambda: native.dot_topk(ta, users, tb, None, 100),
             "dot_rank_mt20": lambda: native.dot_rank(ta, users, tb, None, tg[20], 20),
             f"dot_rank_mt{cap}": lambda: native.dot_rank(ta, users, tb, None, tg[cap], cap),
             "unfused_rank_rows_mt1": lambda: rank_of_items(m, users, tg[1], fused=False, max_targets=1)}
    us = _interleaved(calls, repeats, {"*": 10 if B == 4096 else 30, "unfused_rank_rows_mt1": 2})
    same = True
    for n in (1, 20):
        a = native.dot_rank(ta, users, tb, None, tg[n], n)
        b = rank_of_items(m, users, tg[n], fused=False, max_targets=n)
        same = same and bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    res = {"readout": "dot", "D": D, "users": B, "items": I, "repeats": repeats, "equal_to_unfused": same}
    res.update(_summary(us, 2.0 * B * I * D))
    return res


def mlp_shape(E, B, repeats):
    from deeprecommendation_amd import native, rank_of_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    dev = torch.device("cuda:0")
    N1, N2 = 256, 128
    torch.manual_seed(E)
    m = BasicNCF(item_dim=I, user_dim=4096, item_emb=E, user_emb=E, mlp_dense_layers=[N1, N2]).to(dev).eval()
    cache = m._refresh()
    packed = m._packed_mlp("MLP", cache)
    ta = m._table("user", m.user_embeddings[0], cache)
    tb = m._table("item", m.item_embeddings[0], cache)
    users = torch.arange(B, device=dev)
    tg = {n: _targets(B, n, dev) for n in (1, 20)}
    calls = {"mlp_topk_k10": lambda: native.mlp_topk(ta, users, tb, None, packed, 10),
             "mlp_rank_mt1": lambda: native.mlp_rank(ta, users, tb, None, packed, tg[1], 1),
             "mlp_rank_mt20": lambda: native.mlp_rank(ta, users, tb, None, packed, tg[20], 20)}
    us = _interleaved(calls, repeats, {"*": 3 if B == 4096 else 10})
    a = native.mlp_rank(ta, users, tb, None, packed, tg[1], 1)
    b = rank_of_items(m, users, tg[1], fused=False, max_targets=1)
    res = {"readout": "mlp", "E": E, "users": B, "items": I, "repeats": repeats,
           "equal_to_unfused": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))}
    res.update(_summary(us, 2.0 * B * I * (E * N1 + N1 * N2 + N2) + 2.0 * B * E * N1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("readout", choices=["dot", "mlp"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", nargs=2, type=int, default=None, help="(child) width and users of the one shape to run")
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    a = ap.parse_args()
    if a.shape is not None:
        fn = dot_shape if a.readout == "dot" else mlp_shape
        print(json.dumps(fn(a.shape[0], a.shape[1], a.repeats)), flush=True)
        return 0
    for w in ((64, 256) if a.readout == "dot" else (64, 128)):
        for B in (512, 4096):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), a.readout, "--repeats", str(a.repeats),
                   "--shape", str(w), str(B)]
            rc = subprocess.call(cmd)
            if rc != 0:                                  # a fault, an abort or the time limit: nothing more is started on the GPU
                print(json.dumps({"readout": a.readout, "shape": [w, B], "failed_with_status": rc}), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
