"""Dev tool (GPU box): times the EASE fit and its full-catalogue top-K on the device against the torch composition; prints ONE JSON
object.

    python tools/ab_ease.py [--users 6040] [--items 3706] [--ratings 1000000] [--zipf 0.5] [--reg 500] [--top 10]
                            [--score-users 4096] [--rounds 3] [--dense-limit-gib 16]
    python tools/ab_ease.py --users 100000 --items 20000 --ratings 5000000 --zipf 0.8

Workload (seeded, tools/ab_knn.py's generator): about ``--ratings`` distinct (user, item) pairs, users uniform, item of popularity
rank r drawn with weight 1 / (r + 1) ** zipf, half-star ratings 0.5 .. 5.  Reported, each the median over ``--rounds`` alternating
rounds after a warm-up, with the spread (max - min) / median, device events around back-to-back launches that end in a synchronise:
  gram_ms             ncf_ease_gram over all rows (the transpose, torch ops, is transpose_ms)
  copy_ms             one (I, I) device copy: the in-place entries below are timed behind one, and it is taken off their figures
  invert_ms           ncf_ease_invert; invert_tflops = 2 I^3 / invert_ms, invert_peak_share against the 157.3 TF fp32 MFMA peak
  weights_ms          ncf_ease_weights
  fit_ms              EASE.fit_csr, everything above together with its check()
  topk_ms             recommend.ease_top_k for ``--score-users`` users against the whole catalogue
  torch_gram_ms / torch_inv_ms / torch_fit_ms / torch_topk_ms
                      the composition where the dense (U, I) matrix fits ``--dense-limit-gib``: X.T @ X, torch.linalg.inv, the
                      elementwise weights; X[users] @ W and torch.topk — else null ("does not fit"); where torch.linalg.inv itself raises,
                      its message is reported as torch_error and serving is timed on the device's weights
  fit_peak_gib        torch's peak allocation over one EASE.fit_csr; torch_fit_peak_gib the composition's (its dense X included)
The composition's sums are in another order: its weights are compared by the largest difference, its lists by their overlap."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deeprecommendation_amd import EASE, ease_top_k, native  # noqa: E402
from deeprecommendation_amd.baselines import build_transpose  # noqa: E402
from ab_knn import timed, workload  # noqa: E402

PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=0.5)
    ap.add_argument("--reg", type=float, default=500.0)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--score-users", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense-limit-gib", type=float, default=16.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I = args.users, args.items
    rowptr, col, val = (torch.from_numpy(a).to(dev) for a in workload(U, I, args.ratings, args.zipf))
    val = (val - val.min() + 0.5).contiguous()                           # the generator centres its ratings; EASE reads them as they are
    nnz = col.numel()
    ratings = (rowptr, col, val)
    score_users = torch.arange(min(args.score_users, U), device=dev)
    colptr, row, tval = build_transpose(rowptr, col, val, I)
    G = native.ease_gram(rowptr, col, val, colptr, row, tval)
    A = torch.empty_like(G)

    def fit():
        return EASE(reg=args.reg).fit_csr(rowptr, col, val, I)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    a = fit()
    fit_peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30
    b = fit()
    repeat_equal = bool(torch.equal(a.weights_, b.weights_))
    del b

    def copy_then(fn):
        def run():
            A.copy_(G)
            return fn(A)
        return run

    runs = {
        "transpose_ms": lambda: build_transpose(rowptr, col, val, I),
        "gram_ms": lambda: native.ease_gram(rowptr, col, val, colptr, row, tval, out=A),
        "copy_ms": copy_then(lambda M: M),
        "invert_ms": copy_then(lambda M: native.ease_invert(M, args.reg)),
        "weights_ms": copy_then(native.ease_weights),
        "fit_ms": fit,
        "topk_ms": lambda: ease_top_k(a, ratings, score_users, args.top),
    }
    dense = U * I * 4 <= args.dense_limit_gib * 2 ** 30
    torch_peak = torch_error = Wt = None
    if dense:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        owner = torch.repeat_interleave(torch.arange(U, device=dev), torch.diff(rowptr))
        X = torch.zeros((U, I), device=dev)
        X[owner, col.long()] = val

        def torch_gram():
            return X.t() @ X

        def torch_inv():
            A.copy_(G)
            A.diagonal().add_(args.reg)
            return torch.linalg.inv(A)

        def torch_fit():
            Gt = X.t() @ X
            Gt.diagonal().add_(args.reg)
            P = torch.linalg.inv(Gt)
            W = P / (-torch.diagonal(P))
            return W.fill_diagonal_(0.0)

        try:
            Wt = torch_fit()
            torch_peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30
            runs.update(torch_inv_ms=torch_inv, torch_fit_ms=torch_fit)
        except RuntimeError as e:                                        # reported as it is: the composition could not invert this size
            torch_error = str(e).splitlines()[0][:200]
            Wt = None
        Ws = a.weights_ if Wt is None else Wt                            # serving is timed on whichever weights there are

        def torch_topk():
            return torch.topk(X[score_users] @ Ws, args.top, dim=1)

        runs.update(torch_gram_ms=torch_gram, torch_topk_ms=torch_topk)
    for fn in runs.values():                                             # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):                                         # alternating, round by round
        for k, fn in runs.items():
            times[k].append(timed(fn)[0])
    a.check()
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    for k in ("invert_ms", "weights_ms"):                                # net of the copy they are timed behind
        med[k] = med[k] - med["copy_ms"]
    if "torch_inv_ms" in med:
        med["torch_inv_ms"] = med["torch_inv_ms"] - med["copy_ms"]
    tflops = 2.0 * I ** 3 / (med["invert_ms"] * 1e-3) / 1e12
    diff = overlap = None
    if Wt is not None:
        diff = float((a.weights_ - Wt).abs().max() / Wt.abs().max())
    if dense:
        mine, theirs = ease_top_k(a, ratings, score_users, args.top)[1], torch_topk()[1]
        overlap = float((mine[:, :, None] == theirs[:, None, :]).any(2).float().mean())
    print(json.dumps({
        "tool": "ab_ease", "device": torch.cuda.get_device_name(dev), "users": U, "items": I, "ratings": nnz, "zipf": args.zipf, "reg": args.reg,
        "top": args.top, "score_users": int(score_users.numel()), "rounds": args.rounds, "panel": native.EASE_BLOCK,
        "panels": -(-I // native.EASE_BLOCK), "most_popular_item_users": int(torch.diff(colptr).max()),
        "longest_user_row": int(torch.diff(rowptr).max()), **med, "torch_gram_ms": med.get("torch_gram_ms"),
        "torch_inv_ms": med.get("torch_inv_ms"), "torch_fit_ms": med.get("torch_fit_ms"), "torch_topk_ms": med.get("torch_topk_ms"),
        "invert_tflops": tflops, "invert_peak_share": tflops / PEAK_TF, "fit_peak_gib": fit_peak, "torch_fit_peak_gib": torch_peak,
        "spread": spread, "dense_fits": dense, "weights_max_diff_vs_torch": diff, "top_overlap_with_torch": overlap,
        "repeat_equal_bits": repeat_equal, "torch_error": torch_error,
    }))


if __name__ == "__main__":
    main()
