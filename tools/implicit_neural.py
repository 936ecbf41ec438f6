"""Implicit-feedback MF (sampled loss and full-catalogue softmax), BasicNCF and NeuMF (from scratch, and initialised from the fitted
MF + BasicNCF by ``NeuMF.from_pretrained``) beside the ImplicitALS baseline, all under one evaluation, on the device.

    python tools/implicit_neural.py RATINGS [--min-rating 0] [--negatives 4] [--loss bce] [--epochs 20] [--batch-size 65536]
                                            [--lr 0.001] [--factors 64] [--candidates 99] [--als-iters 15] [--seed 0]
                                            [--softmax-scale 1.0]

RATINGS is a sample file (CSV with userId, movieId, rating and, optionally, timestamp columns; ``.csv`` may be left off).  Every
rating of at least ``--min-rating`` is an interaction.  ``leave_one_out`` holds out one item per user (the latest with a timestamp
column, a seeded pick without), the rest trains: MF, BasicNCF and the two NeuMF by ``fit_implicit`` (``--negatives`` unseen items per positive, redrawn
every epoch on the device), a second MF by ``fit_implicit(loss="softmax")`` (each positive against the whole catalogue, no
negatives; ``--softmax-scale`` multiplies the logits), ImplicitALS by its own solver on the same pairs with value 1.  Each model is then reported twice: by
``eval_sampled`` (the held-out item among ``--candidates`` sampled unseen items, the same lists for every model) and by
``eval_full_ranking`` (the held-out item against the whole catalogue, the training items left out)."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import (ImplicitALS, ImplicitFeedback, eval_full_ranking, eval_sampled, fit_implicit, leave_one_out,  # noqa: E402
                                    sampled_candidates)
from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.neumf import NeuMF  # noqa: E402


def fmt(m):
    return f"HR@10 {m['hr@10']:.4f}, NDCG@10 {m['ndcg@10']:.4f}, MRR {m['mrr']:.4f}, AUC {m['auc']:.4f} ({int(m['users'])} users)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ratings")
    ap.add_argument("--min-rating", type=float, default=0.0)
    ap.add_argument("--negatives", type=int, default=4)
    ap.add_argument("--loss", choices=["bce", "bpr"], default="bce")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=65536)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--factors", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=99)
    ap.add_argument("--als-iters", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--softmax-scale", type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = args.ratings if os.path.exists(args.ratings) else args.ratings + ".csv"
    frame = pd.read_csv(path)
    frame = frame[frame["rating"] >= args.min_rating]
    user_ids, u = np.unique(frame["userId"].to_numpy(), return_inverse=True)
    item_ids, i = np.unique(frame["movieId"].to_numpy(), return_inverse=True)
    n_users, n_items = len(user_ids), len(item_ids)
    stamps = frame["timestamp"].to_numpy() if "timestamp" in frame.columns else None
    tu, ti, hu, hi = leave_one_out(u, i, stamps, seed=args.seed)
    print(f"{n_users} users, {n_items} items, {len(tu)} training pairs, {len(hu)} held-out items "
          f"({'latest interaction' if stamps is not None else 'seeded pick'})", flush=True)
    data = ImplicitFeedback(tu, ti, n_users, n_items, dev)
    users, held = torch.from_numpy(hu).to(dev), torch.from_numpy(hi).to(dev)
    candidates = sampled_candidates(data, users, held, n_candidates=args.candidates, seed=args.seed)
    targets = (torch.arange(len(hu) + 1, dtype=torch.int64, device=dev), held.to(torch.int32))
    exclude = data.exclusion(users)

    def report(name, model):
        model.eval()                                                   # the full-catalogue functions score in eval mode only
        print(f"{name}: sampled ({args.candidates} candidates) {fmt(eval_sampled(model, users, held, candidates))}", flush=True)
        print(f"{name}: full catalogue {fmt(eval_full_ranking(model, users, targets, exclude=exclude, cutoffs=(10,)))}", flush=True)

    torch.manual_seed(args.seed)
    F = args.factors
    fitted = {}
    # the paper's table: its two ablations (MF as GMF, BasicNCF as the MLP tower), then NeuMF from scratch and NeuMF initialised from
    # the two fitted ablations (its Eq. 13, alpha = 0.5)
    for name, make in (("MF", lambda: MF(item_dim=n_items, user_dim=n_users, item_emb=F, user_emb=F)),
                       ("BasicNCF", lambda: BasicNCF(item_dim=n_items, user_dim=n_users, item_emb=F, user_emb=F, mlp_dense_layers=[2 * F, F])),
                       ("NeuMF", lambda: NeuMF(item_dim=n_items, user_dim=n_users, mf_dim=F, item_emb=F, user_emb=F,
                                               mlp_dense_layers=[2 * F, F])),
                       ("NeuMF pretrained", lambda: NeuMF.from_pretrained(fitted["MF"], fitted["BasicNCF"], alpha=0.5)),
                       ("MF softmax", lambda: MF(item_dim=n_items, user_dim=n_users, item_emb=F, user_emb=F))):
        model = fitted[name] = make()
        def on_epoch(epoch, m, name=name):
            print(f"{name} epoch {epoch + 1}: sampled HR@10 {eval_sampled(m, users, held, candidates)['hr@10']:.4f}", flush=True)
        loss = "softmax" if name == "MF softmax" else args.loss
        hist = fit_implicit(model, data, negatives=args.negatives, loss=loss, epochs=args.epochs, batch_size=args.batch_size,
                            lr=args.lr, seed=args.seed, on_epoch=on_epoch, scale=args.softmax_scale)
        print(f"{name}: train loss {hist['train_loss'][0]:.4f} -> {hist['train_loss'][-1]:.4f}")
        report(name, model)
    als = ImplicitALS(n_factors=F, n_iters=args.als_iters)
    als.fit(data.users, data.items, torch.ones(len(data), dtype=torch.float32, device=dev), n_users, n_items,
            generator=torch.Generator().manual_seed(args.seed))
    report("ImplicitALS", als.as_mf())


if __name__ == "__main__":
    main()
