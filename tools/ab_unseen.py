"""Dev tool (GPU box): times ncf_sample_unseen against the torch composition it replaces; prints ONE JSON object.

    python tools/ab_unseen.py [--shapes ml1m big] [--batch 65536] [--k-train 4] [--k-eval 99] [--rounds 5] [--reps 20]

Shapes (seeded): ``ml1m`` 6040 users x 3706 items with 1 M positives (item of popularity rank r drawn with weight 1 / (r + 1) ** 0.5),
``big`` 100 000 x 20 000 with 5 M positives (weight 1 / (r + 1): Zipf).  Two workloads per shape:
  train   one epoch's negatives: the positives in a seeded permutation, batches of ``--batch`` users, ``--k-train`` draws each
  eval    ``--k-eval`` candidates for every user in one call
Two sides, the same users in the same order:
  kernel  native.sample_unseen: one launch per batch, no host read
  torch   torch.randint over the catalogue, a membership test by torch.searchsorted on the sorted user * n_items + item keys, and
          redraw rounds of the draws that hit a seen item until none is left; each round reads the number left on the host.  It does
          NOT make a row's draws distinct (the kernel does): it is the cheaper job.
Reported per (shape, workload, side): the median milliseconds over ``--rounds`` alternating rounds after a warm-up — device events
around a window that ends in a synchronise; the kernel's window repeats its work ``--reps`` times and is divided by it, so that it is
not a window of microseconds — with the spread (max - min) / median, and for torch the redraw rounds and host reads of one pass.  Both
sides' outputs are checked: no draw is a seen item, and the kernel's rows hold distinct items."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402

SHAPES = {"ml1m": (6040, 3706, 1_000_000, 0.5), "big": (100_000, 20_000, 5_000_000, 1.0)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out      # ms


def workload(users, items, positives, zipf, seed=11):
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(items) + 1.0) ** zipf
    draws = int(positives * 1.6)
    key = np.unique(rng.integers(0, users, draws) * items + rng.choice(items, draws, p=w / w.sum()))
    return np.sort(rng.permutation(key)[:positives])


def torch_draw(keys, users, n_items, K, counters):
    """The composition: (n, K) unseen items of ``users``; counters += (redraw rounds, host reads)."""
    n = users.numel()
    out = torch.randint(0, n_items, (n, K), device=users.device)
    base = (users * n_items)[:, None].expand(n, K)
    flat, fbase = out.view(-1), base.reshape(-1)
    todo = torch.arange(n * K, device=users.device)
    while True:
        k = fbase[todo] + flat[todo]
        pos = torch.searchsorted(keys, k).clamp_max(keys.numel() - 1)
        todo = todo[keys[pos] == k]
        counters[1] += 1
        if todo.numel() == 0:            # the size of todo: a host read
            return out
        counters[0] += 1
        flat[todo] = torch.randint(0, n_items, (todo.numel(),), device=users.device)


def unseen_ok(keys, users, n_items, out):
    k = (users * n_items)[:, None] + out
    pos = torch.searchsorted(keys, k.reshape(-1)).clamp_max(keys.numel() - 1)
    return bool((keys[pos] != k.reshape(-1)).all()) and bool(((out >= 0) & (out < n_items)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--k-train", type=int, default=4)
    ap.add_argument("--k-eval", type=int, default=99)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for name in args.shapes:
        U, I, P, zipf = SHAPES[name]
        key = workload(U, I, P, zipf)
        keys = torch.from_numpy(key).to(dev)
        pu, pi = keys // I, keys % I
        rowptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(pu, minlength=U), 0)
        seen = (rowptr, pi.to(torch.int32))
        order = torch.from_numpy(np.random.default_rng(5).permutation(len(key))).to(dev)
        epoch_users = pu[order].contiguous()
        all_users = torch.arange(U, device=dev)
        longest = int(torch.diff(rowptr).max())
        for workload_name, users, K, B in (("train", epoch_users, args.k_train, args.batch), ("eval", all_users, args.k_eval, U)):
            n = users.numel()
            batches = [(s, users[s:s + B].contiguous()) for s in range(0, n, B)]
            out = torch.empty((n, K), dtype=torch.int64, device=dev)

            def kernel_once():
                for s, u in batches:
                    native.sample_unseen(seen, I, u, K, 17, s, out=out[s:s + u.numel()])
                return out

            def kernel():
                for _ in range(args.reps):
                    kernel_once()

            counters = [0, 0]

            def composition():
                return [torch_draw(keys, u, I, K, counters) for _, u in batches]

            kernel_once(), composition()                                       # warm-up of every shape the timed windows use
            torch.cuda.synchronize()
            native.check_unseen(dev)
            ok_kernel = unseen_ok(keys, users, I, out) and bool((torch.sort(out, 1).values.diff(dim=1) > 0).all())
            ok_torch = all(unseen_ok(keys, u, I, o) for (_, u), o in zip(batches, composition()))
            times = {"kernel": [], "torch": []}
            per_pass = []
            for _ in range(args.rounds):                                       # alternating, round by round
                times["kernel"].append(timed(kernel)[0] / args.reps)
                counters[:] = [0, 0]
                times["torch"].append(timed(composition)[0])
                per_pass.append(tuple(counters))
            med = {k: statistics.median(v) for k, v in times.items()}
            results.append({
                "shape": name, "users": U, "items": I, "positives": len(key), "longest_row": longest, "workload": workload_name, "k": K,
                "rows": n, "launches": len(batches), "kernel_ms": med["kernel"], "torch_ms": med["torch"],
                "torch_over_kernel": med["torch"] / med["kernel"],
                "spread": {k: (max(v) - min(v)) / med[k] for k, v in times.items()},
                "torch_redraw_rounds": statistics.median(c[0] for c in per_pass), "torch_host_reads": statistics.median(c[1] for c in per_pass),
                "kernel_host_reads": 0, "kernel_draws_unseen_and_distinct": ok_kernel, "torch_draws_unseen": ok_torch,
            })
    print(json.dumps({"tool": "ab_unseen", "device": torch.cuda.get_device_name(dev), "batch": args.batch, "rounds": args.rounds,
                      "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
