"""Dev tool (GPU box): times the ItemKNN fit and its full-catalogue top-K on the device against the torch composition; prints ONE
JSON object.

    python tools/ab_knn.py [--users 6040] [--items 3706] [--ratings 1000000] [--zipf 0.5] [--k 50] [--shrink 10] [--top 10]
                           [--score-users 4096] [--rounds 3] [--dense-limit-gib 4]

Workload (seeded): about ``--ratings`` distinct (user, item) pairs, users uniform, item of popularity rank r drawn with weight
1 / (r + 1) ** zipf, half-star ratings centred on their mean.  Reported, each the median over ``--rounds`` alternating rounds after a
warm-up, with the spread (max - min) / median, device events around calls that end in a synchronise:
  fit_ms              ItemKNN.fit_csr: transpose (torch), ncf_knn_item_sq, ncf_knn_sim_rows + ncf_topk_rows per block of rows
  sim_rows_ms         the ncf_knn_sim_rows launches of those blocks alone
  chain_ms            ncf_knn_sim_rows for the ONE most popular item: its users are one serial chain, the floor of a fit however the
                      other items are scheduled; chain_share = chain_ms / sim_rows_ms
  topk_ms             recommend.item_knn_top_k for ``--score-users`` users against the whole catalogue
  torch_fit_ms        the composition where the dense (U, I) matrix fits ``--dense-limit-gib``: X.T @ X, the co-rating counts M.T @ M,
                      elementwise shrunk cosines, torch.topk — else null ("does not fit")
  torch_topk_ms       dense (users, I) @ (I, I) products of the neighbour weights for numerator and denominator, a division, torch.topk
The composition's sums are in another order: its table is compared by the overlap of neighbour sets, not by bits."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import ItemKNN, item_knn_top_k, native  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out      # ms


def workload(users, items, ratings, zipf, seed=11):
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(items) + 1.0) ** zipf
    key = np.unique(rng.integers(0, users, int(ratings * 1.6)) * items + rng.choice(items, int(ratings * 1.6), p=w / w.sum()))
    key = np.sort(rng.permutation(key)[:ratings])
    u, i = key // items, key % items
    r = rng.integers(1, 11, len(key)) * 0.5
    rowptr = np.zeros(users + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(u, minlength=users))
    return rowptr, i.astype(np.int32), (r - r.mean()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=0.5)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--shrink", type=float, default=10.0)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--score-users", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense-limit-gib", type=float, default=4.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I = args.users, args.items
    rowptr, col, val = (torch.from_numpy(a).to(dev) for a in workload(U, I, args.ratings, args.zipf))
    nnz = col.numel()
    model = ItemKNN(k=args.k, shrink=args.shrink)
    colptr, row, tval = model.build_transpose(rowptr, col, val, I)
    per_item = torch.diff(colptr)
    top_item = int(per_item.argmax())
    sq = native.knn_item_sq(colptr, tval)
    rows = max(1, min(native.KNN_MAX_ROWS, (256 << 20) // (4 * I)))
    blocks = [(i0, min(I, i0 + rows)) for i0 in range(0, I, rows)]
    buf = torch.empty((rows, I), dtype=torch.float32, device=dev)
    score_users = torch.arange(min(args.score_users, U), device=dev)
    ratings = (rowptr, col, val)

    def fit():
        return ItemKNN(k=args.k, shrink=args.shrink).fit_csr(rowptr, col, val, I)

    def sim_rows():
        for i0, i1 in blocks:
            native.knn_sim_rows(rowptr, col, val, colptr, row, tval, sq, (i0, i1), 1, args.shrink, out=buf[:i1 - i0])

    def chain():
        native.knn_sim_rows(rowptr, col, val, colptr, row, tval, sq, (top_item, top_item + 1), 1, args.shrink, out=buf[:1])

    dense = U * I * 4 <= args.dense_limit_gib * 2 ** 30
    if dense:
        owner = torch.repeat_interleave(torch.arange(U, device=dev), torch.diff(rowptr))
        X = torch.zeros((U, I), device=dev)
        M = torch.zeros((U, I), device=dev)
        X[owner, col.long()], M[owner, col.long()] = val, 1.0

    def torch_fit():
        G, co = X.t() @ X, M.t() @ M
        n = torch.sqrt(torch.diagonal(G))
        S = G / (n[:, None] * n[None, :]) * (co / (co + args.shrink))
        S = torch.where((co >= 1) & (S > 0), S, torch.zeros_like(S)).fill_diagonal_(0.0)
        return torch.topk(S, args.k, dim=1)

    a = fit()
    b = fit()
    repeat_equal = bool(torch.equal(a.nb_pos_, b.nb_pos_) and torch.equal(a.nb_sim_, b.nb_sim_) and torch.equal(a.nb_cnt_, b.nb_cnt_))

    def topk():
        return item_knn_top_k(a, ratings, score_users, args.top)

    def torch_topk():
        Wt = torch.zeros((I, I), device=dev)
        live = a.nb_pos_ >= 0
        src = torch.arange(I, device=dev)[:, None].expand_as(a.nb_pos_)[live]
        Wt[a.nb_pos_[live].long(), src] = a.nb_sim_[live]               # Wt[j, i] = s_ij
        num, den = X[score_users] @ Wt, M[score_users] @ Wt
        return torch.topk(torch.where(den > 0, num / den, torch.zeros_like(num)), args.top, dim=1)

    runs = {"fit_ms": fit, "sim_rows_ms": sim_rows, "chain_ms": chain, "topk_ms": topk}
    if dense:
        runs.update(torch_fit_ms=torch_fit, torch_topk_ms=torch_topk)
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
    overlap = None
    if dense:
        tp = torch_fit()[1]
        tv = torch_fit()[0] > 0
        hit = ((a.nb_pos_[:, :, None] == tp[:, None, :]) & tv[:, None, :]).any(2) & (a.nb_pos_ >= 0)
        overlap = float(hit.sum()) / max(1, int((a.nb_pos_ >= 0).sum()))
    print(json.dumps({
        "tool": "ab_knn", "device": torch.cuda.get_device_name(dev), "users": U, "items": I, "ratings": nnz, "zipf": args.zipf, "k": args.k,
        "shrink": args.shrink, "top": args.top, "score_users": int(score_users.numel()), "rounds": args.rounds,
        "most_popular_item_users": int(per_item.max()), "longest_user_row": int(torch.diff(rowptr).max()), "item_blocks": len(blocks),
        **med, "torch_fit_ms": med.get("torch_fit_ms"), "torch_topk_ms": med.get("torch_topk_ms"),
        "chain_share": med["chain_ms"] / med["sim_rows_ms"], "spread": spread, "dense_fits": dense, "neighbour_overlap_with_torch": overlap,
        "mean_neighbours": float(a.nb_cnt_.float().mean()), "repeat_equal_bits": repeat_equal,
    }))


if __name__ == "__main__":
    main()
