"""Dev tool (GPU box): times the KernelMF fit (ncf_kmf_epoch, stratified SGD) on the device; prints ONE JSON object.

    python tools/ab_kmf.py [--ratings 3000000] [--users 200000] [--items 50000] [--factors 128] [--blocks 0] [--epochs 2] [--rounds 3]

Workload (seeded): ``--ratings`` half-star ratings of uniformly drawn users and Zipf-skewed items (item of rank k with weight
1 / (k + 1)), F = ``--factors``, W = ``--blocks`` (0: the device's CU count).  Nothing else on the device fits this model, so there is
no second route to compare with; what is reported is where an epoch's time goes:
  ms_per_epoch              ``--epochs`` epochs in one ncf_kmf_epoch call (W launches each), device events around the call, after a
                            warm-up call; the median over ``--rounds`` rounds and the spread (max - min) / median
  ms_per_epoch_empty_plan   the same call over a plan of the same W whose blocks are all empty: W launches per epoch that walk no
                            sample — what an epoch pays for being W dependent launches (launch gaps and empty waves)
  launch_share              ms_per_epoch_empty_plan / ms_per_epoch
  us_per_sample_chain       one wave walking a chain: a W = 1 fit over the first ``--chain`` samples (one block, one launch per epoch),
                            time per sample
  longest_chain             samples of the largest block of each stratum (a launch ends when its longest chain does): mean and max
                            over the strata, the balanced size n / W^2, and the mean times us_per_sample_chain
The fit is checked for the kernel's flags and for equal bits over two runs from the same start."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import KernelMF, native  # noqa: E402

LR, REG = 0.001, 0.01


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)      # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratings", type=int, default=3_000_000)
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=50_000)
    ap.add_argument("--factors", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = args.blocks or torch.cuda.get_device_properties(dev).multi_processor_count
    F, n = args.factors, args.ratings
    rng = np.random.default_rng(11)
    weights = 1.0 / (np.arange(args.items) + 1.0)
    user = torch.from_numpy(rng.integers(0, args.users, n)).to(dev)
    item = torch.from_numpy(rng.choice(args.items, n, p=weights / weights.sum())).to(dev)
    rating = torch.from_numpy((rng.integers(1, 11, n) * 0.5).astype(np.float32)).to(dev)
    mu = float(np.float32(rating.double().sum().item() / n))

    model = KernelMF(n_factors=F, n_blocks=W)
    plan = model.build_plan(user, item, rating, args.users, args.items, W)
    ld = (F + 1 + 31) // 32 * 32
    g = torch.Generator(device=dev).manual_seed(3)
    start = [torch.zeros((rows, ld), device=dev) for rows in (args.users, args.items)]
    for t in start:
        t[:, :F].normal_(0.0, 0.1, generator=g)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def epochs(p, tables, e):
        return native.kmf_epoch(tables[0], tables[1], F, p["user"], p["item"], p["rating"], p["block_ptr"], p["user_block"], p["item_block"],
                                mu, LR, REG, e, flag=flag)

    empty = dict(plan, block_ptr=torch.zeros_like(plan["block_ptr"]))
    chain_n = min(args.chain, n)
    one = model.build_plan(user[:chain_n], item[:chain_n], rating[:chain_n], args.users, args.items, 1)
    a, b = [t.clone() for t in start], [t.clone() for t in start]
    sse_a, sse_b = epochs(plan, a, args.epochs), epochs(plan, b, args.epochs)         # also the warm-up of the full plan
    epochs(empty, [t.clone() for t in start], 1)
    epochs(one, [t.clone() for t in start], 1)
    torch.cuda.synchronize()
    repeat_equal = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(sse_a, sse_b))
    rmse = [float(v) for v in torch.sqrt(sse_a.sum(1) / n).cpu()]
    work = [t.clone() for t in start]
    times = {"full": [], "empty": [], "chain": []}
    for _ in range(args.rounds):                                      # alternating, round by round
        times["full"].append(timed(lambda: epochs(plan, work, args.epochs)) / args.epochs)
        times["empty"].append(timed(lambda: epochs(empty, work, args.epochs)) / args.epochs)
        times["chain"].append(timed(lambda: epochs(one, work, 1)))
    flags = int(flag.item())
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    sizes = torch.diff(plan["block_ptr"]).view(W, W)                  # [stratum, block]
    longest = sizes.max(1).values.double()
    us_per_sample = med["chain"] * 1e3 / chain_n
    print(json.dumps({
        "tool": "ab_kmf", "device": torch.cuda.get_device_name(dev), "ratings": n, "users": args.users, "items": args.items, "F": F, "W": W,
        "epochs_per_call": args.epochs, "rounds": args.rounds, "ms_per_epoch": med["full"], "ms_per_epoch_empty_plan": med["empty"],
        "launch_share": med["empty"] / med["full"], "spread": spread, "chain_samples": chain_n, "us_per_sample_chain": us_per_sample,
        "longest_chain": {"mean_samples": float(longest.mean()), "max_samples": float(longest.max()), "balanced_samples": n / (W * W),
                          "mean_us": float(longest.mean()) * us_per_sample,
                          "sum_over_strata_ms": float(longest.sum()) * us_per_sample * 1e-3},
        "samples_per_second": n / (med["full"] * 1e-3), "train_rmse": rmse, "flags": flags, "repeat_equal_bits": repeat_equal,
    }))


if __name__ == "__main__":
    main()
