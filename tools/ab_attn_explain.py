"""Dev tool (GPU box): explanations for many users' winners, two routes alternating in one process; prints ONE JSON object.

    python tools/ab_attn_explain.py [--rounds 5] [--window 0.5] [--users 4096]

Workload: BASELINE config 3's model (F = 2094, A = 128, MLP [256, 128], IE = UE = 64; the attention's output layer scaled so that its
softmax is not flat), a catalogue of 1174 items, 4096 users with about 300 ratings each (seeded), k = 10 winners per user from
top_k_items (outside the timed windows), E = 8 reasons.  Routes:
  (a) dense    what exists without ncf_attn_explain: forward(..., return_attention_weights=True) on blocks of (user, winner) pairs —
               a dense (pairs, I_c) weight block —, then the threshold and a stable descending sort in torch, the first E kept
  (b) table    explain_items: the cached logit table + one ncf_attn_explain launch (the table's build is timed separately)
Each timed window is device events around repetitions that end in a synchronise, at least ``--window`` seconds long, after a warm-up
of every route; the routes alternate round by round; reported: the median over the rounds, the spread (max - min) / median, the
dense route's peak device bytes above the resident state, and how far the two routes' results agree."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import explain_items, native, top_k_items  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF, RowsOf, SparseRatings  # noqa: E402

I_CAT, F_DIM, A_ATT, EMB, K, E = 1174, 2094, 128, 64, 10, 8
MEAN_RATED, GAIN = 300, 200.0
FACTOR, CONSTANT = 1.5, 0.025
DENSE_BLOCK_PAIRS = 4096                 # a (4096, 1174) fp32 weight block is 19 MB


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


def workload(dev, users):
    torch.manual_seed(7)
    model = AttentionNCF(item_dim=F_DIM, item_emb=EMB, user_emb=EMB, att_dense=A_ATT, mlp_dense_layers=[256, 128]).eval()
    with torch.no_grad():
        model.AttentionNet[-1].weight.mul_(GAIN)
    model.to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    feats = (torch.rand(I_CAT, F_DIM, device=dev, generator=g) < 0.02).float()
    lens = torch.randint(MEAN_RATED - 100, MEAN_RATED + 101, (users,), generator=torch.Generator().manual_seed(11))
    rowptr = torch.zeros(users + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, 0)
    # each user's columns: the first n of a random order of the catalogue, ascending (one argsort of random keys, no per-user loop)
    order = torch.rand(users, I_CAT, device=dev, generator=g).argsort(1)
    take = torch.arange(I_CAT, device=dev)[None] < lens.to(dev)[:, None]
    member = torch.zeros(users, I_CAT, dtype=torch.bool, device=dev).scatter_(1, order, take)
    col = member.nonzero()[:, 1].to(torch.int32)
    val = torch.randint(1, 11, (int(rowptr[-1]),), device=dev, generator=g).float() * 0.5 - 2.9
    return model, feats, SparseRatings(rowptr.to(dev), col, val, I_CAT), lens


def dense_route(model, feats, ratings, users, winners, thr):
    """(positions (B, k, E) int64, weights (B, k, E), counts (B, k) int32) through the dense weight blocks."""
    B, k = winners.shape
    flat_w, flat_u = winners.reshape(-1), users.repeat_interleave(k)
    flat_t = thr.repeat_interleave(k)
    pos, wts, cnt = [], [], []
    with torch.no_grad():
        for p0 in range(0, B * k, DENSE_BLOCK_PAIRS):
            p1 = min(B * k, p0 + DENSE_BLOCK_PAIRS)
            pairs = SparseRatings(ratings.rowptr, ratings.col, ratings.val, I_CAT, pair_row=flat_u[p0:p1])
            _, dense = model(RowsOf(feats, flat_w[p0:p1]), feats, pairs, return_attention_weights=True)
            ok = dense > flat_t[p0:p1, None]                         # an unrated item's weight is 0, below every threshold
            w, idx = torch.sort(torch.where(ok, dense, torch.full_like(dense, -1.0)), dim=1, descending=True, stable=True)
            w, idx = w[:, :E], idx[:, :E]
            pos.append(torch.where(w >= 0, idx, torch.full_like(idx, -1)))
            wts.append(w.clamp_min(0.0))
            cnt.append(ok.sum(1).to(torch.int32))
    return torch.cat(pos).view(B, k, E), torch.cat(wts).view(B, k, E), torch.cat(cnt).view(B, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--users", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, feats, ratings, lens = workload(dev, args.users)
    users = torch.arange(args.users, dtype=torch.int64, device=dev)
    _, winners, counts = top_k_items(model, users, K, profiles=(feats, ratings))
    assert int(counts.min()) == K
    thr = (FACTOR / lens.clamp_min(1).float() + CONSTANT).to(dev)

    dense = lambda: dense_route(model, feats, ratings, users, winners, thr)
    table = lambda: explain_items(model, users, winners, (feats, ratings), max_reasons=E, explain_factor=FACTOR, explain_constant=CONSTANT)

    def build():
        model._refresh().pop("cross_table", None)
        with torch.no_grad():
            model.logit_table(feats)

    with torch.no_grad():
        ST = model.logit_table(feats)
    out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in (((args.users, K, E), torch.int32), ((args.users, K, E), torch.float32),
                                                                   ((args.users, K, E), torch.float32), ((args.users, K), torch.int32)))
    kernel = lambda: native.attn_explain(ST, ratings.rowptr, ratings.col, ratings.val, users, winners, thr, E, out=out)
    routes = {"dense": dense, "table": table, "table_build": build, "attn_explain_kernel": kernel}
    for fn in routes.values():                                        # warm-up of each route
        fn()
        fn()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    d_pos, d_w, d_cnt = dense()
    torch.cuda.synchronize()
    dense_peak = torch.cuda.max_memory_allocated(dev) - resident
    torch.cuda.reset_peak_memory_stats(dev)
    ex = table()
    torch.cuda.synchronize()
    table_peak = torch.cuda.max_memory_allocated(dev) - resident
    times = {k: [] for k in routes}
    for _ in range(args.rounds):                                      # alternating, round by round
        for name, fn in routes.items():
            times[name].append(window(fn, args.window if name != "table_build" else args.window / 4))
    native.check_oob(dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    # agreement: pairs whose counts and listed positions are equal; the rest should hold a weight within 1e-4 (relative) of the threshold or of
    # another listed weight (the two routes sum in different orders)
    same = (d_cnt == ex.counts) & (d_pos == ex.positions).all(2)
    listed = d_pos >= 0
    cells = float(lens.sum()) * K                                     # (entry, winner) logits: each is looked up once in the table
    print(json.dumps({
        "tool": "ab_attn_explain", "device": torch.cuda.get_device_name(dev), "users": args.users, "k": K, "E": E, "items": I_CAT,
        "rated_entries": int(lens.sum()), "rounds": args.rounds, "seconds": med, "spread": spread,
        "speedup_table_over_dense": med["dense"] / med["table"],
        "dense_peak_bytes": int(dense_peak), "table_peak_bytes": int(table_peak), "dense_block_pairs": DENSE_BLOCK_PAIRS,
        "dense_full_matrix_bytes": 4 * args.users * K * I_CAT, "logit_table_bytes": 4 * I_CAT * I_CAT,
        "kernel_table_cells_per_second": cells / med["attn_explain_kernel"],
        "pairs": args.users * K, "pairs_equal": int(same.sum()), "mean_count": float(ex.counts.float().mean()),
        "max_count": int(ex.counts.max()),
        "max_weight_diff_on_equal_pairs": float(((d_w - ex.weights).abs() * (same[:, :, None] & listed)).max()),
    }))


if __name__ == "__main__":
    main()
