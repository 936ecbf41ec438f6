"""Dev tool (GPU box): times the MMR re-ranking kernel (ncf_mmr_rerank) against a torch composition; prints ONE JSON object.

    python tools/ab_mmr.py [--rounds 21] [--warmup 3] [--shapes 128,64,20 256,128,20 256,256,20] [--batches 4096 256]

Workload (seeded): per shape (N, D, K) and batch B, pools of N distinct items out of 16 * N unit-norm Gaussian item vectors with
uniform scores, lambda = 0.5, min-max relevance.  Two routes over the same device tensors, alternating round by round after
``--warmup`` untimed rounds, device events around each; the median over ``--rounds`` rounds and the spread (max - min) / median:
  kernel     native.mmr_rerank: one launch
  torch      the composition this kernel replaces: gather the pool's rows (B, N, D), one bmm for the (B, N, N) Gram tensor, then K
             rounds of masked arg-max / gather / maximum (about 5 K launches)
and per route the peak of torch's allocator above what the inputs hold (the kernel route: its three outputs).  ``picks_equal`` is the
share of users whose K picks are the same on both routes (the composition sums a similarity in another order, so near-ties may
differ); ``repeat_equal_bits`` holds two kernel launches together.  ``kernel_gmacs`` = B * (K - 1) * N * D multiply-adds over the
kernel's time."""
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out      # ms


def torch_mmr(vec, score, pos, K, lam):
    """The composition: Gram tensor, then K masked arg-max rounds.  Returns the picked slots (B, K) int64."""
    B, N = score.shape
    rows = vec[pos]                                               # (B, N, D)
    gram = torch.bmm(rows, rows.transpose(1, 2))                  # (B, N, N)
    lo, hi = score.min(1, keepdim=True).values, score.max(1, keepdim=True).values
    rel = torch.where(hi == lo, torch.zeros_like(score), (score - lo) / (hi - lo))
    m = torch.full_like(score, float("-inf"))
    open_ = torch.ones_like(score, dtype=torch.bool)
    picks = torch.empty((B, K), dtype=torch.int64, device=score.device)
    for t in range(K):
        v = rel if t == 0 else lam * rel - (1.0 - lam) * m
        s = torch.where(open_, v, torch.full_like(v, float("-inf"))).argmax(1, keepdim=True)
        picks[:, t:t + 1] = s
        open_.scatter_(1, s, False)
        m = torch.maximum(m, gram.gather(2, s[:, :, None].expand(B, N, 1)).squeeze(2))
    return picks


def peak_above(base, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["128,64,20", "256,128,20", "256,256,20"])
    ap.add_argument("--batches", nargs="+", type=int, default=[4096, 256])
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error("--rounds: the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    lam = 0.5
    results = []
    for shape in args.shapes:
        N, D, K = (int(x) for x in shape.split(","))
        if not native.mmr_supported(N, D, K):
            ap.error(f"--shapes {shape}: outside the kernel's envelope")
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(N * 1000 + D + B)
            vec = torch.nn.functional.normalize(torch.randn((16 * N, D), device=dev, generator=g), dim=1)
            score = torch.rand((B, N), device=dev, generator=g)
            pos = torch.rand((B, 16 * N), device=dev, generator=g).argsort(1)[:, :N].contiguous()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            kernel = lambda: native.mmr_rerank(vec, score, pos, None, K, lam, True)
            compo = lambda: torch_mmr(vec, score, pos, K, lam)
            peak_k, a = peak_above(base, kernel)
            peak_t, picks_t = peak_above(base, compo)
            b = kernel()
            torch.cuda.synchronize()
            repeat_equal = all(torch.equal(x, y) for x, y in zip(a, b))
            picks_equal = float((a[0].to(torch.int64) == picks_t).all(1).double().mean())
            for _ in range(args.warmup):
                kernel(), compo()
            torch.cuda.synchronize()
            times = {"kernel": [], "torch": []}
            for _ in range(args.rounds):                              # alternating, round by round
                times["kernel"].append(timed(kernel)[0])
                times["torch"].append(timed(compo)[0])
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
            results.append({"N": N, "D": D, "K": K, "B": B, "kernel_ms": med["kernel"], "torch_ms": med["torch"], "spread": spread,
                            "torch_over_kernel": med["torch"] / med["kernel"], "kernel_peak_bytes": peak_k, "torch_peak_bytes": peak_t,
                            "kernel_gmacs": B * (K - 1) * N * D / (med["kernel"] * 1e-3) * 1e-9, "picks_equal": picks_equal,
                            "repeat_equal_bits": repeat_equal})
            native.check_oob(dev)
    print(json.dumps({"tool": "ab_mmr", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "warmup": args.warmup, "lam": lam,
                      "results": results}))


if __name__ == "__main__":
    main()
