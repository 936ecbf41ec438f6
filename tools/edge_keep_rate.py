"""Dev tool (GPU box): the measurements of DESIGN §4.26 — node / message dropout of the GraphNCF training step drawn on the device.

    python tools/edge_keep_rate.py [part ...]        parts: kernel, step (default: both)

  kernel  ncf_edge_keep + ncf_edge_coef on the cfg-4 graph (1 M users x 100 k items, 50 M interactions = 100 M directed edges, Zipf items),
          back to back (HIP events): bytes read + written per second beside a live ncf_probe_copy of the same volume, for the pair and for
          each kernel alone; batch of 65 536 target pairs, message dropout 0.1, with and without a node mask, and without targets
  step    one GraphNCF / LightGCN training step (2 layers, hetero, D = 64, MLP [256, 128], default dropout_rate, message_dropout 0.1,
          batch 4096, FusedAdam) on the toy interaction recipe scaled to 500 000 interactions (about 10^6 directed edges): the HIP path
          with the edge set drawn by ncf_edge_keep against the same step with train_with_torch_ops = True (F.dropout on the host, boolean
          compaction, per-edge Linear + index_add_), interleaved windows in one process
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphData, GraphNCF, PreparedGraph  # noqa: E402
from deeprecommendation_amd.optim import FusedAdam  # noqa: E402


def events_us(fn, reps, settle=3):
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def cfg4_graph(dev):
    """bench_extra._cfg4_graph: Zipf(1) item popularity, uniform users, ratings as weights."""
    I, U, n = 100_000, 1_000_000, 50_000_000
    g = torch.Generator(device=dev).manual_seed(11)
    p = 1.0 / torch.arange(1, I + 1, device=dev, dtype=torch.float64)
    items = torch.multinomial((p / p.sum()).float(), n, replacement=True, generator=g)
    users = torch.randint(0, U, (n,), device=dev, generator=g) + I
    attr = torch.randint(1, 11, (n,), device=dev, generator=g).float() * 0.5 - 3.0
    return GraphData(user2item_edge_index=torch.stack([users, items]), item2user_edge_index=torch.stack([items, users]),
                     user2item_edge_attr=attr, item2user_edge_attr=attr.clone(), num_items=I, num_users=U)


def copy_ceiling(dev, nbytes, reps):
    """GB/s read + written of a live ncf_probe_copy that moves ``nbytes`` in all."""
    half = nbytes // 2 // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    lib = native.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    us = events_us(lambda: native._check(lib.ncf_probe_copy(src.data_ptr(), dst.data_ptr(), half, st)), reps)
    return 2 * half / us / 1e3


def part_kernel(dev):
    graph = cfg4_graph(dev)
    prep = PreparedGraph(graph, hetero=True)
    dst_of, src, pair_key, slot = prep.train_state()
    E, N, B = prep.col.numel(), prep.N, 65_536
    g = torch.Generator(device=dev).manual_seed(3)
    pick = torch.randint(0, E // 2, (B,), device=dev, generator=g)
    users, items = graph.user2item_edge_index[0][pick], graph.user2item_edge_index[1][pick]
    targets = torch.sort(users * N + items).values.contiguous()
    node_keep = GraphNCF._draw_node_keep(N, users, items, 0.1, 777)
    n_seg = prep.segptr.numel() - 1
    print(f"cfg-4 graph: {E} CSR entries, {N} rows, {n_seg} level-0 segments (mean {E / n_seg:.1f} entries each), {B} target pairs", flush=True)
    coef_bytes = E * 24                                # src 8 + dst 8 + w 4 read, coef 4 written (the degree gathers hit in cache)
    for name, tg, nk in (("message 0.1 + targets", targets, None), ("message 0.1 + targets + node mask", targets, node_keep),
                         ("message 0.1, no targets (what the per-lane target search costs)", None, None)):
        seeds = [0]
        # col 4 + slot 4 + attr 4 read, w 4 written, pair_key 8 only under target masking; segptr; deg cleared (node mask: cached)
        keep_bytes = E * (16 + (8 if tg is not None else 0)) + n_seg * 8 + N * 4

        def keep():
            seeds[0] += 1
            return native.edge_keep(prep.segptr, prep.row_of, N, prep.col, prep.attr, pair_key, tg, slot, 0.1, seeds[0], nk)

        w, deg = keep()
        degf = deg.to(torch.float32)

        def coef():
            return native.edge_coef(src, dst_of, w, degf)

        def both():
            ww, dd = keep()
            return native.edge_coef(src, dst_of, ww, dd.to(torch.float32))

        res = {"pair": [], "edge_keep": [], "edge_coef": [], "copy": []}
        for _ in range(3):                               # alternate: box noise shows in the spread
            res["pair"].append(events_us(both, 10))
            res["edge_keep"].append(events_us(keep, 10))
            res["edge_coef"].append(events_us(coef, 10))
            res["copy"].append(copy_ceiling(dev, keep_bytes + coef_bytes, 10))
        pair, k_us, c_us, ceil = min(res["pair"]), min(res["edge_keep"]), min(res["edge_coef"]), max(res["copy"])
        rate = (keep_bytes + coef_bytes) / pair / 1e3
        print(f"{name}: edge_keep + edge_coef {pair:.0f} us = {rate:.0f} GB/s read + written; live copy ceiling {ceil:.0f} GB/s: "
              f"{rate / ceil:.2f} of it.  edge_keep alone {k_us:.0f} us = {keep_bytes / k_us / 1e3:.0f} GB/s, edge_coef alone {c_us:.0f} us = "
              f"{coef_bytes / c_us / 1e3:.0f} GB/s; kept fraction {float((w != 0).float().mean()):.4f}  (all runs: {res})", flush=True)
    # what it replaces on the no-dropout path, for scale: masked_coef (isin / bincount / pow over all E entries)
    us = events_us(lambda: prep.masked_coef(users, items), 5, settle=2)
    print(f"masked_coef (torch ops, targets only) on the same graph and batch: {us:.0f} us", flush=True)


def toy_graph(dev, n=500_000, U=25_000, I=10_000, seed=0):
    """The toy interaction recipe of the training tests (uniform users and items, rating = a function of both + noise), scaled up."""
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    r = np.clip(np.round(((u % 5) + (i % 3)) * 0.5 + 1 + rng.normal(0, 0.2, n), 1), 0.5, 5.0).astype(np.float32)
    users, items = torch.from_numpy(u + I).to(dev), torch.from_numpy(i).to(dev)
    attr = torch.from_numpy(r - r.mean()).to(dev)
    graph = GraphData(user2item_edge_index=torch.stack([users, items]), item2user_edge_index=torch.stack([items, users]),
                      user2item_edge_attr=attr, item2user_edge_attr=attr.clone(), num_items=I, num_users=U)
    return graph, users, items, torch.from_numpy(r).to(dev).view(-1, 1)


def part_step(dev):
    graph, users, items, y = toy_graph(dev)
    I, U, B = graph.num_items, graph.num_users, 4096
    n = users.numel()
    steps = {}
    for mode in ("hip", "torch_ops"):
        torch.manual_seed(0)
        model = GraphNCF(item_dim=I, user_dim=U, num_gnn_layers=2, hetero=True, node_emb=64, mlp_dense_layers=[256, 128],
                         message_dropout=0.1).to(dev).train()
        model.train_with_torch_ops = mode == "torch_ops"
        opt = FusedAdam(model.parameters(), lr=1e-3)
        k = [0]

        def step(model=model, opt=opt, k=k):
            s = (k[0] * B) % (n - B)
            k[0] += 1
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.mse_loss(model(graph, users[s:s + B], items[s:s + B], dev, True), y[s:s + B], reduction="sum")
            loss.backward()
            opt.step()

        steps[mode] = step
    res = {"hip": [], "torch_ops": []}
    for _ in range(3):                                   # interleaved windows
        for mode in ("hip", "torch_ops"):
            res[mode].append(events_us(steps[mode], 10, settle=3))
    h, t = min(res["hip"]), min(res["torch_ops"])
    print(f"GraphNCF / LightGCN step, {2 * n} directed edges, batch {B}, message_dropout 0.1: HIP path with ncf_edge_keep {h / 1e3:.2f} ms, "
          f"torch ops {t / 1e3:.2f} ms: {t / h:.1f}x  (all runs, us: {res})", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("edge_keep_rate.py measures on a GPU; none found")
    dev = torch.device("cuda:0")
    for p in sys.argv[1:] or ["kernel", "step"]:
        {"kernel": part_kernel, "step": part_step}[p](dev)


if __name__ == "__main__":
    main()
