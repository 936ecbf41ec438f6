"""Dev tool (GPU box): times the ImplicitALS half-sweeps on the device against the torch composition; prints ONE JSON object.

    python tools/ab_als.py [--users 6040] [--items 3706] [--ratings 1000000] [--zipf 0.5] [--factors 64] [--reps 5] [--rounds 3]
                           [--torch-reps 1] [--chunk-mib 512]

Workload (seeded, the one of tools/ab_knn.py): about ``--ratings`` distinct (user, item) pairs, users uniform, item of popularity
rank r drawn with weight 1 / (r + 1) ** zipf, half-star values.  Both tables are N(0, 0.1) draws: a half-sweep's time does not
depend on the values.  Reported in ms per call, steady state: after a warm-up of every timed shape, device events around ``--reps``
back-to-back calls, the median over ``--rounds`` alternating rounds with the spread (max - min) / median:
  user_sweep_ms       ncf_als_gram of the item table + ncf_als_solve_rows over every user (the plan built once, outside)
  item_sweep_ms       the same over the transposed CSR against the user table: the popular items are the long rows
  gram_ms             ncf_als_gram of the larger table alone
  longest_row_ms      ncf_als_solve_rows for the ONE longest row of the transposed CSR (its segment workgroups, then its own
                      workgroup, whose right-hand side is one serial sum over the row): the floor of that half-sweep however the
                      other rows are scheduled; longest_row_share = longest_row_ms / item_sweep_ms
  torch_user_sweep_ms the composition for the user half-sweep: T^T T, the dense (rows, F, F) normal matrices built chunk by chunk
                      (``--chunk-mib`` of them at a time; the outer products of a chunk's entries added with index_add_), then
                      torch.linalg.cholesky and torch.cholesky_solve
The composition's sums are in another order: its rows are compared by the largest difference, not by bits."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deeprecommendation_amd import native  # noqa: E402
from deeprecommendation_amd.baselines import build_transpose  # noqa: E402
from ab_knn import workload  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out      # ms per call


def torch_sweep(rowptr, rowptr_host, col, val, T, alpha, reg, chunk_bytes):
    """x_u = (T^T T + sum (alpha v) t t^T + reg I)^-1 sum (1 + alpha v) t for every row, by dense torch operations."""
    R, F = rowptr.numel() - 1, T.shape[1]
    base = T.t() @ T + reg * torch.eye(F, device=T.device)
    out = torch.empty((R, F), device=T.device)
    rows = max(1, chunk_bytes // (4 * F * F))
    owner = torch.repeat_interleave(torch.arange(R, device=T.device), rowptr[1:] - rowptr[:-1])
    w = alpha * val
    for r0 in range(0, R, rows):
        r1 = min(R, r0 + rows)
        A = base.expand(r1 - r0, F, F).contiguous()
        e0, e1 = int(rowptr_host[r0]), int(rowptr_host[r1])
        for s0 in range(e0, e1, rows):                                 # as many outer products at a time as normal matrices
            s1 = min(e1, s0 + rows)
            t = T[col[s0:s1].long()]
            A.index_add_(0, owner[s0:s1] - r0, (w[s0:s1, None] * t)[:, :, None] * t[:, None, :])
        b = torch.zeros((r1 - r0, F), device=T.device)
        b.index_add_(0, owner[e0:e1] - r0, (1.0 + w[e0:e1, None]) * T[col[e0:e1].long()])
        out[r0:r1] = torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--ratings", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=0.5)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--reg", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk-mib", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I, F = args.users, args.items, args.factors
    host = workload(U, I, args.ratings, args.zipf)
    rowptr, col, val = (torch.from_numpy(a).to(dev) for a in host)
    val = val - val.min() + 0.5                                        # ab_knn centres its values; a confidence needs them >= 0
    colptr, row, tval = build_transpose(rowptr, col, val, I)
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.empty((U, F), device=dev).normal_(0.0, 0.1, generator=g)
    Y = torch.empty((I, F), device=dev).normal_(0.0, 0.1, generator=g)
    users, items = torch.arange(U, device=dev), torch.arange(I, device=dev)
    plan_u, plan_i = native.als_plan(rowptr, users, F), native.als_plan(colptr, items, F)
    per_item = torch.diff(colptr)
    longest = per_item.argmax().view(1)
    plan_l = native.als_plan(colptr, longest, F)
    out_u, out_i, out_l = torch.empty((U, F), device=dev), torch.empty((I, F), device=dev), torch.empty((1, F), device=dev)
    big = X if U >= I else Y

    def user_sweep():
        return native.als_solve_rows(rowptr, col, val, users, Y, native.als_gram(Y), args.alpha, args.reg, out=out_u, plan=plan_u)

    def item_sweep():
        return native.als_solve_rows(colptr, row, tval, items, X, native.als_gram(X), args.alpha, args.reg, out=out_i, plan=plan_i)

    GX = native.als_gram(X)

    def longest_row():
        return native.als_solve_rows(colptr, row, tval, longest, X, GX, args.alpha, args.reg, out=out_l, plan=plan_l)

    def gram():
        return native.als_gram(big)

    def torch_user_sweep():
        return torch_sweep(rowptr, host[0], col, val, Y, args.alpha, args.reg, args.chunk_mib << 20)

    runs = {"user_sweep_ms": (user_sweep, args.reps), "item_sweep_ms": (item_sweep, args.reps), "gram_ms": (gram, args.reps),
            "longest_row_ms": (longest_row, args.reps), "torch_user_sweep_ms": (torch_user_sweep, args.torch_reps)}
    for fn, _ in runs.values():                                        # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    a = user_sweep().clone()
    repeat_equal = bool(torch.equal(a, user_sweep()))
    diff = float((a - torch_user_sweep()).abs().max())
    times = {k: [] for k in runs}
    for _ in range(args.rounds):                                       # alternating, round by round
        for k, (fn, reps) in runs.items():
            times[k].append(timed(fn, reps)[0])
    native.check_als(dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    print(json.dumps({
        "tool": "ab_als", "device": torch.cuda.get_device_name(dev), "users": U, "items": I, "ratings": int(col.numel()), "zipf": args.zipf,
        "factors": F, "reps": args.reps, "rounds": args.rounds, "longest_user_row": int(torch.diff(rowptr).max()),
        "longest_item_row": int(per_item.max()), "item_rows_over_one_segment": int((per_item > native.ALS_SEG).sum()),
        "item_scratch_slots": sum(p[4] for p in plan_i), "item_batches": len(plan_i), **med,
        "longest_row_share": med["longest_row_ms"] / med["item_sweep_ms"], "torch_over_device": med["torch_user_sweep_ms"] / med["user_sweep_ms"],
        "spread": spread, "max_abs_difference_from_torch": diff, "max_abs_solution": float(a.abs().max()), "repeat_equal_bits": repeat_equal,
    }))


if __name__ == "__main__":
    main()
