"""Dev tool (GPU box): one GraphNCF / LightGAT training step on the HIP blocks against the same step on the torch ops
(``train_with_torch_ops = True``), alternating in one process; prints ONE JSON object.

    python tools/ab_gat_train.py [--rounds 5] [--window 0.5] [--users 100000] [--items 10000] [--interactions 500000]

Workload: 2 LightGAT layers, hetero, D = 64, MLP [256, 128], one-hot node features, default dropout_rate (per-(edge, feature)
dropout 0.1 inside the per-edge Linear), batch 4096, target edges masked; a bipartite graph of ``interactions`` distinct (user, item)
pairs = 2 x that many directed edges, the item side drawn as U^2 (a Zipf-like head: the most popular items have thousands of
in-edges, so their rows are split into 512-entry segments), edge weights N(0, 1).  The step is forward + mse loss + backward with the
gradients cleared; each configuration runs without and with message_dropout = 0.1 (the torch path then draws its E-sized mask on the
host).  Each timed window is device events around repetitions that end in a synchronise, at least ``--window`` seconds long, after a
warm-up of both routes; the two routes alternate and swap their order round by round; reported: the median over the rounds, the
spread (max - min) / median, and the ratio of the medians.  With every dropout off the two routes compute the same loss: its relative
difference is reported too."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd.neural_collaborative_filtering.models.gnn_ncf import GraphData, GraphNCF  # noqa: E402

D, LAYERS, BATCH = 64, 2, 4096


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


def workload(dev, U, I, n):
    g = torch.Generator().manual_seed(7)
    key = torch.unique(torch.randint(0, U, (n,), generator=g) * I + (torch.rand(n, generator=g) ** 2 * I).long())
    u, i = key // I + I, key % I
    a = torch.randn(u.numel(), generator=g)
    graph = GraphData(user2item_edge_index=torch.stack([u, i]).to(dev), item2user_edge_index=torch.stack([i, u]).to(dev),
                      user2item_edge_attr=a.to(dev), item2user_edge_attr=a.clone().to(dev), num_items=I, num_users=U)
    pick = torch.randint(0, u.numel(), (BATCH,), generator=g)
    return graph, u[pick].to(dev), i[pick].to(dev), (torch.rand(BATCH, 1, generator=g) * 5).to(dev)


def run(dev, args, message_dropout):
    graph, users, items, y = workload(dev, args.users, args.items, args.interactions)
    torch.manual_seed(3)
    base = GraphNCF(item_dim=args.items, user_dim=args.users, num_gnn_layers=LAYERS, hetero=True, node_emb=D, mlp_dense_layers=[256, 128],
                    message_dropout=message_dropout, convType="LightGAT").to(dev).train()
    m_hip, m_torch = copy.deepcopy(base), copy.deepcopy(base)
    m_torch.train_with_torch_ops = True

    def step(m):
        def fn():
            for q in m.parameters():
                q.grad = None
            loss = torch.nn.functional.mse_loss(m(graph, users, items, dev, True), y, reduction="sum")
            loss.backward()
            return loss
        return fn

    routes = {"hip": step(m_hip), "torch": step(m_torch)}
    for fn in routes.values():                                        # warm-up of each route (graph preparation, code objects)
        fn()
        fn()
    torch.cuda.synchronize()
    prep = graph._prepared[("prep", True)]
    times = {k: [] for k in routes}
    for r in range(args.rounds):                                      # alternating, the order swapped round by round
        for name in (("hip", "torch") if r % 2 == 0 else ("torch", "hip")):
            times[name].append(window(routes[name], args.window))
    med = {k: statistics.median(v) for k, v in times.items()}
    # same loss with every dropout off
    quiet = copy.deepcopy(base)
    quiet.message_dropout = None
    for mod in quiet.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    twin = copy.deepcopy(quiet)
    twin.train_with_torch_ops = True
    l_hip, l_torch = float(step(quiet)().detach()), float(step(twin)().detach())
    E = int(prep.col.numel())
    return {"message_dropout": message_dropout, "users": args.users, "items": args.items, "directed_edges": E, "D": D, "layers": LAYERS,
            "batch": BATCH, "segments": int(prep.segptr.numel() - 1), "longest_row": int(prep.counts.max()), "rows_split": prep.row_of is not None,
            "rounds": args.rounds, "seconds": med, "spread": {k: (max(v) - min(v)) / med[k] for k, v in times.items()},
            "torch_over_hip": med["torch"] / med["hip"], "loss_hip": l_hip, "loss_torch": l_torch,
            "loss_rel_diff_without_dropout": abs(l_hip - l_torch) / abs(l_torch)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--items", type=int, default=10000)
    ap.add_argument("--interactions", type=int, default=500000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"tool": "ab_gat_train", "device": torch.cuda.get_device_name(dev),
                      "configs": [run(dev, args, md) for md in (None, 0.1)]}))


if __name__ == "__main__":
    main()
