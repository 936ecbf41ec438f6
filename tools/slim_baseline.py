"""The sparse item-item baseline of a full-catalogue ranking evaluation on the device: SLIM chosen by validation NDCG@10.

    python tools/slim_baseline.py TRAIN VAL TEST [--l1 1 5 20] [--l2 10 50 200] [--signed] [--binary] [--min-rating 0]
                                                 [--max-sweeps 100] [--tol 1e-4] [--warm-path]

TRAIN / VAL / TEST are the sample files (CSV with userId, movieId, rating columns; ``.csv`` may be left off).  Every rating of at
least ``--min-rating`` is an interaction, held with its rating (with 1.0 under ``--binary``); a pair listed twice keeps its last
rating.  Grid search over (l1, l2), every l1 with every l2: the Gram matrix of TRAIN is computed once (``fit_csr(at_regs=...)``),
every grid point is one coordinate descent per item and prints the density of its weights, the sweeps of its slowest column, the
columns that met ``--max-sweeps`` and the full-catalogue HR@10, NDCG@10, MRR and AUC of VAL's items (``slim_ranks``, every item of
the catalogue ranked, the user's TRAIN items left out).  The grid point with the best validation NDCG@10 is then scored on TEST the
same way, from the users' TRAIN rows, with the TRAIN and the VAL items left out.  Users of VAL / TEST without a TRAIN interaction
score 0 everywhere.  ``--warm-path`` starts every grid point from the one before it (the grid runs l1 descending inside l2
descending): faster, but a point's bits then depend on the path."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deeprecommendation_amd import SLIM, held_out_items, ranking_metrics, rated_exclusion, slim_ranks  # noqa: E402
from implicit_baseline import Ratings, csr_of, fmt, read_samples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("train"), ap.add_argument("val"), ap.add_argument("test")
    ap.add_argument("--l1", type=float, nargs="+", default=[1.0, 5.0, 20.0])
    ap.add_argument("--l2", type=float, nargs="+", default=[10.0, 50.0, 200.0])
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--binary", action="store_true")
    ap.add_argument("--min-rating", type=float, default=0.0)
    ap.add_argument("--max-sweeps", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--warm-path", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = [read_samples(p) for p in (args.train, args.val, args.test)]
    lookups, counts = [], []
    for column in ("userId", "movieId"):
        ids = pd.unique(pd.concat([f[column] for f in frames]))
        lookups.append(pd.Series(np.arange(len(ids), dtype=np.int64), index=ids))
        counts.append(len(ids))
    (lu, li), (n_users, n_items) = lookups, counts
    train = csr_of(frames[:1], lu, li, n_users, n_items, args.min_rating, dev)
    seen_at_test = csr_of(frames[:2], lu, li, n_users, n_items, args.min_rating, dev)

    def held(frame):
        frame = frame[frame["rating"] >= args.min_rating]
        return held_out_items(frame, lambda ids: lu.loc[ids].to_numpy(), lambda ids: li.loc[ids].to_numpy(), device=dev)

    def metrics(model, users, targets, seen):
        rank, ranked = slim_ranks(model, train, users, targets, exclude=seen)
        model.check()
        return ranking_metrics(rank, targets[0], ranked, cutoffs=(10,))

    val_users, val_targets = held(frames[1])
    test_users, test_targets = held(frames[2])
    val_seen = rated_exclusion(Ratings(train[0], train[1]), val_users)
    grid = [(l1, l2) for l2 in sorted(args.l2, reverse=True) for l1 in sorted(args.l1, reverse=True)]
    proto = SLIM(grid[0][0], grid[0][1], positive=not args.signed, max_sweeps=args.max_sweeps, tol=args.tol, binary=args.binary)
    best = None
    for model in proto.fit_csr(*train, n_items, at_regs=grid, warm_path=args.warm_path):
        m = metrics(model, val_users, val_targets, val_seen)
        print(f"l1={model.l1_reg} l2={model.l2_reg} positive={model.positive} binary={model.binary}: density {model.density_:.4f}, "
              f"sweeps <= {int(model.sweeps_.max())}, unconverged {model.n_unconverged_}; val {fmt(m)}", flush=True)
        if best is None or m["ndcg@10"] > best[0]["ndcg@10"]:
            best = (m, model)
    m, model = best
    print(f"best by val NDCG@10: l1={model.l1_reg} l2={model.l2_reg} positive={model.positive} binary={model.binary} "
          f"(val NDCG@10 {m['ndcg@10']:.4f})")
    test_seen = rated_exclusion(Ratings(seen_at_test[0], seen_at_test[1]), test_users)
    print(f"test {fmt(metrics(model, test_users, test_targets, test_seen))}")


if __name__ == "__main__":
    main()
