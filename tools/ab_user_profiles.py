"""Dev tool (GPU box): the content form of BasicNCF at the reference's own size; prints ONE JSON object.

    python tools/ab_user_profiles.py [--users 20000] [--rounds 5] [--window 0.5] [--numpy-users 1024]

Workload (seeded): a catalogue of 3706 items with F = 1200 feature columns, ``--users`` users (the reference's data sets have about
5 000 to 160 000) with 100 .. 500 half-star ratings each, BasicNCF(F, F, emb 64 / 64, MLP [256, 128]).  Three comparisons:
  (1) profiles   native.user_profiles (one launch for every user) against the reference's loop — create_user_embedding: per user
                 ((r - avg).reshape(-1, 1) * feat[col]).mean(axis=0) in numpy float64 — timed on the first ``--numpy-users`` users and
                 scaled to all of them; the kernel also against the bytes it reads: 4 F per rating from the feature table (which the
                 Infinity Cache holds), 8 per rating of col and rating, 4 F written per user.  The two agree bit for bit (checked here
                 on the timed users).
  (2) forward    one indexed forward (set_content: positions into the cached content . W^T + b tables) against the float-row
                 forward of the same pairs — with the (B, F) rows ready on the device, and including their gather from the content
                 tables — B = 65 536 pairs.  The table build (once per weight version) is timed on its own.
  (3) top-K      top_k_items for 4096 users, k = 20, every item: the fused route (ncf_mlp_topk over the content tables) against
                 fused=False (score blocks through the indexed forward, then ncf_topk_rows); equal bits (checked).
Each timed window is device events around repetitions that end in a synchronise, at least ``--window`` seconds long, after a warm-up
of every route; the routes alternate round by round; reported: the median over the rounds and the spread (max - min) / median."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native, top_k_items  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF  # noqa: E402

I_CAT, F_DIM, EMB, K = 3706, 1200, 64, 20
MIN_RATED, MAX_RATED = 100, 500
PAIRS, TOPK_USERS = 65536, 4096


def window(fn, seconds):
    """Seconds per call of ``fn`` over one window of at least ``seconds``: events around the repetitions, then a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, int(seconds / max(e0.elapsed_time(e1) * 1e-3, 1e-6)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def workload(users):
    rng = np.random.default_rng(7)
    want = rng.integers(MIN_RATED, MAX_RATED + 1, users)
    # each user's columns: every item with the user's own probability, ascending (row lengths scatter a little around ``want``)
    member = rng.random((users, I_CAT), dtype=np.float32) < (want / I_CAT)[:, None].astype(np.float32)
    member[:, 0] |= ~member.any(axis=1)
    lens = member.sum(axis=1)
    rowptr = np.zeros(users + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.nonzero(member)[1].astype(np.int32)
    rating = (rng.integers(1, 11, int(rowptr[-1])) * 0.5).astype(np.float32)
    mean = np.add.reduceat(rating.astype(np.float64), rowptr[:-1]) / lens
    feat = (rng.standard_normal((I_CAT, F_DIM)) * (rng.random((I_CAT, F_DIM)) < 0.05)).astype(np.float32)
    return rowptr, col, rating, (mean + 2.5) / 2, feat


def numpy_loop(rowptr, col, rating, avg, feat64, n):
    out = np.zeros((n, feat64.shape[1]), dtype=np.float32)
    for u in range(n):
        beg, end = rowptr[u], rowptr[u + 1]
        out[u] = ((rating[beg:end].astype(np.float64) - avg[u]).reshape(-1, 1) * feat64[col[beg:end]]).mean(axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--numpy-users", type=int, default=1024)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, rating, avg, feat = workload(args.users)
    nnz = int(rowptr[-1])
    d = [torch.from_numpy(a).to(dev) for a in (rowptr, col, rating, avg, feat)]
    out = torch.empty((args.users, F_DIM), dtype=torch.float32, device=dev)
    profiles = lambda: native.user_profiles(*d, out=out)

    n_np = min(args.numpy_users, args.users)
    feat64 = feat.astype(np.float64)
    numpy_loop(rowptr, col, rating, avg, feat64, min(n_np, 8))
    t0 = time.perf_counter()
    ref = numpy_loop(rowptr, col, rating, avg, feat64, n_np)
    numpy_seconds = time.perf_counter() - t0
    prof = profiles().clone()
    torch.cuda.synchronize()
    bit_equal = bool(torch.equal(prof[:n_np].cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32)))

    torch.manual_seed(7)
    model = BasicNCF(item_dim=F_DIM, user_dim=F_DIM, item_emb=EMB, user_emb=EMB, mlp_dense_layers=[256, 128]).eval().to(dev)
    feat_d = d[4]
    model.set_content(prof, feat_d)
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, args.users, (PAIRS,), generator=g).to(dev)
    i = torch.randint(0, I_CAT, (PAIRS,), generator=g).to(dev)
    rows_u, rows_i = prof[u], feat_d[i]
    tk_users = torch.randint(0, args.users, (TOPK_USERS,), generator=g).to(dev)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def build():
        model._native_ver = None
        model._table("user", model.user_embeddings[0])
        model._table("item", model.item_embeddings[0])

    routes = {
        "profiles_kernel": profiles,
        "forward_indexed": no_grad(lambda: model(u, i)),
        "forward_float_rows": no_grad(lambda: model(rows_u, rows_i)),
        "forward_float_rows_with_gather": no_grad(lambda: model(prof[u], feat_d[i])),
        "topk_fused": lambda: top_k_items(model, tk_users, K),
        "topk_unfused": lambda: top_k_items(model, tk_users, K, fused=False),
        "table_build": no_grad(build),
    }
    for fn in routes.values():                                        # warm-up of each route
        fn()
        fn()
    torch.cuda.synchronize()
    fused, unfused = routes["topk_fused"](), routes["topk_unfused"]()
    topk_equal = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                     for a, b in zip(fused, unfused))
    with torch.no_grad():
        fwd_diff = float((model(u, i) - model(rows_u, rows_i)).abs().max())
        fwd_scale = float(model(rows_u, rows_i).abs().max())
    repeat_equal = bool(torch.equal(profiles().view(torch.int32), prof.view(torch.int32)))
    times = {k: [] for k in routes}
    for _ in range(args.rounds):                                      # alternating, round by round
        for name, fn in routes.items():
            times[name].append(window(fn, args.window if name != "table_build" else args.window / 4))
    native.check_oob(dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    chunks = -(-F_DIM // 256)                                         # waves per user: each reads the row's col / rating once
    kernel_bytes = nnz * (4 * F_DIM + 8 * chunks) + args.users * (4 * F_DIM + 24 * chunks)
    numpy_all = numpy_seconds / n_np * args.users
    print(json.dumps({
        "tool": "ab_user_profiles", "device": torch.cuda.get_device_name(dev), "users": args.users, "items": I_CAT, "F": F_DIM,
        "ratings": nnz, "rounds": args.rounds, "seconds": med, "spread": spread,
        "numpy_users_timed": n_np, "numpy_seconds_timed": numpy_seconds, "numpy_seconds_scaled_to_all_users": numpy_all,
        "speedup_kernel_over_numpy": numpy_all / med["profiles_kernel"], "kernel_equals_numpy_bits": bit_equal,
        "kernel_repeat_equal_bits": repeat_equal,
        "kernel_bytes_read_and_written": kernel_bytes, "kernel_bytes_per_second": kernel_bytes / med["profiles_kernel"],
        "kernel_fp64_flop_per_second": 2.0 * nnz * F_DIM / med["profiles_kernel"],
        "pairs": PAIRS, "speedup_indexed_over_float_rows": med["forward_float_rows"] / med["forward_indexed"],
        "speedup_indexed_over_float_rows_with_gather": med["forward_float_rows_with_gather"] / med["forward_indexed"],
        "forward_max_abs_diff": fwd_diff, "forward_max_abs": fwd_scale,
        "topk_users": TOPK_USERS, "k": K, "speedup_topk_fused_over_unfused": med["topk_unfused"] / med["topk_fused"],
        "topk_routes_equal_bits": topk_equal,
    }))


if __name__ == "__main__":
    main()
