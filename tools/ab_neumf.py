"""A/B of the NeuMF kernels.  Every figure is the per-call time of a window of back-to-back launches between one pair of
HIP events, after warm-up: the median of --reps windows, the routes of a comparison taking turns (ab_ms).

    python tools/ab_neumf.py [--reps 7]

  1. neumf_score against the three-launch composition (score_fused + a torch weighted dot + add) at B = 65 536,
     towers 128-128-64 and 128-256-128, D = 32 and 64;
  2. neumf_topk (k = 10) against mlp_topk at the same tower: the price of the GMF term, expected near (EB + D) / EB.  mlp_topk is
     this build's: its kernels are instruction for instruction those of the commit before NeuMF (tools/asm_kernel_diff.py, DESIGN
     4.41), and a library of that commit cannot be loaded beside this binding, which binds the NeuMF symbols at load;
  3. neumf_topk against score-then-select (neumf_score over user blocks + topk_rows) with the peak memory of both, at
     6040 x 3706 and at 100 000 x 20 000 with 4096 users.
Whichever route loses is marked LOSES."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402


def ab_ms(fns, calls, windows, warmup=3):
    """Per-call milliseconds of each route of ``fns``: a window is ``calls`` back-to-back launches between ONE pair of HIP events
    (nothing synchronises inside it, so the queue stays full and a route of several launches is not charged an idle start per
    launch); the routes take turns window by window, so drift hits them alike; the median of ``windows`` windows per route."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(windows):
        for n, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) / calls)
    return [statistics.median(t) for t in times]


def verdict(ours, other):
    return "wins" if ours < other else "LOSES"


def case(dev, tower, D, n_users, n_items, seed=0):
    g = torch.Generator().manual_seed(seed)
    K0, N1, N2 = tower
    dims = [K0, N1] + ([N2] if N2 else []) + [1]
    ws = [(torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5).to(dev) for i in range(len(dims) - 1)]
    bs = [(0.1 * torch.randn(dims[i + 1], generator=g)).to(dev) for i in range(len(dims) - 1)]
    E = K0 // 2
    tabs = [torch.randn(n, e, generator=g).to(dev) for n, e in ((n_users, E), (n_items, E), (n_users, D), (n_items, D))]
    return tabs, native.PackedMLP(ws, bs), torch.randn(D, generator=g).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per route")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 65536
    print("1. pair scorer at B = 65 536 (ms): neumf_score | score_fused + weighted dot + add")
    for tower in ((128, 128, 64), (128, 256, 128)):
        for D in (32, 64):
            tabs, packed, w = case(dev, tower, D, 100000, 20000)
            g = torch.Generator().manual_seed(1)
            u, i = torch.randint(0, 100000, (B,), generator=g).to(dev), torch.randint(0, 20000, (B,), generator=g).to(dev)
            fused, comp, tower_ms = ab_ms([
                lambda: native.neumf_score(tabs[0], u, tabs[1], i, tabs[2], tabs[3], packed, w),
                lambda: native.score_fused(tabs[0], u, tabs[1], i, packed) + ((tabs[2][u] * w) * tabs[3][i]).sum(1, keepdim=True),
                lambda: native.score_fused(tabs[0], u, tabs[1], i, packed)], 200, args.reps)
            print(f"   {tower} D={D}: {fused:.3f} | {comp:.3f}  neumf_score {verdict(fused, comp)}  (score_fused alone: {tower_ms:.3f})")
    print("2. neumf_topk against mlp_topk, k = 10, 4096 users x 20 000 items (ms)")
    for tower in ((128, 128, 64), (128, 256, 128)):
        for D in (32, 64):
            tabs, packed, w = case(dev, tower, D, 100000, 20000)
            users = torch.arange(4096, device=dev)
            neumf = lambda: native.neumf_topk(tabs[0], users, tabs[1], None, tabs[2], tabs[3], packed, w, 10)
            ours, base = ab_ms([neumf, lambda: native.mlp_topk(tabs[0], users, tabs[1], None, packed, 10)], 3, args.reps)
            E = tower[0] // 2
            print(f"   {tower} D={D}: {ours:.3f} | {base:.3f}  ratio {ours / base:.3f}, item-row bytes (EB + D) / EB = {(E + D) / E:.3f}")
    print("3. neumf_topk against score-then-select, k = 10, tower 128-128-64, D = 32 (ms | peak MiB over the tables)")
    for n_users, n_items, rows in ((6040, 3706, 6040), (100000, 20000, 4096)):
        tabs, packed, w = case(dev, (128, 128, 64), 32, n_users, n_items)
        users = torch.arange(rows, device=dev)
        items = torch.arange(n_items, device=dev)

        def select(block=1024):
            out = []
            for b0 in range(0, rows, block):
                ub = users[b0:b0 + block]
                s = native.neumf_score(tabs[0], ub.repeat_interleave(n_items), tabs[1], items.repeat(ub.numel()), tabs[2], tabs[3], packed, w)
                out.append(native.topk_rows(s.view(ub.numel(), n_items), 10))
            return out

        routes = [lambda: native.neumf_topk(tabs[0], users, tabs[1], None, tabs[2], tabs[3], packed, w, 10), select]
        peaks = []
        for fn in routes:                        # peak memory of one call of each route, apart from the timing
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peaks.append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        res = list(zip(ab_ms(routes, 3, args.reps), peaks))
        (a, am), (b, bm) = res
        print(f"   {rows} users x {n_items} items: {a:.2f} | {b:.2f} ms, {am:.0f} | {bm:.0f} MiB  neumf_topk {verdict(a, b)} on time, "
              f"{verdict(am, bm)} on memory")


if __name__ == "__main__":
    main()
