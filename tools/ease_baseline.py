"""The closed-form baseline of a full-catalogue ranking evaluation on the device: EASE chosen by validation NDCG@10.

    python tools/ease_baseline.py TRAIN VAL TEST [--regs 50 100 250 500 1000 2500] [--binary] [--min-rating 0]

TRAIN / VAL / TEST are the sample files (CSV with userId, movieId, rating columns; ``.csv`` may be left off).  Every rating of at
least ``--min-rating`` is an interaction, held with its rating (with 1.0 under ``--binary``); a pair listed twice keeps its last
rating.  Grid search over reg: the Gram matrix of TRAIN is computed once (``fit_csr(at_regs=...)``), every grid point is one
inversion and prints the full-catalogue HR@10, NDCG@10, MRR and AUC of VAL's items (``ease_ranks``, every item of the catalogue
ranked, the user's TRAIN items left out).  The grid point with the best validation NDCG@10 is then scored on TEST the same way, from
the users' TRAIN rows, with the TRAIN and the VAL items left out.  Users of VAL / TEST without a TRAIN interaction score 0 everywhere."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deeprecommendation_amd import EASE, ease_ranks, held_out_items, ranking_metrics, rated_exclusion  # noqa: E402
from implicit_baseline import Ratings, csr_of, fmt, read_samples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("train"), ap.add_argument("val"), ap.add_argument("test")
    ap.add_argument("--regs", type=float, nargs="+", default=[50.0, 100.0, 250.0, 500.0, 1000.0, 2500.0])
    ap.add_argument("--binary", action="store_true")
    ap.add_argument("--min-rating", type=float, default=0.0)
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
        rank, ranked = ease_ranks(model, train, users, targets, exclude=seen)
        model.check()
        return ranking_metrics(rank, targets[0], ranked, cutoffs=(10,))

    val_users, val_targets = held(frames[1])
    test_users, test_targets = held(frames[2])
    val_seen = rated_exclusion(Ratings(train[0], train[1]), val_users)
    best = None
    for model in EASE(binary=args.binary).fit_csr(*train, n_items, at_regs=args.regs):
        m = metrics(model, val_users, val_targets, val_seen)
        print(f"reg={model.reg} binary={model.binary}: val {fmt(m)}", flush=True)
        if best is None or m["ndcg@10"] > best[0]["ndcg@10"]:
            best = (m, model)
    m, model = best
    print(f"best by val NDCG@10: reg={model.reg} binary={model.binary} (val NDCG@10 {m['ndcg@10']:.4f})")
    test_seen = rated_exclusion(Ratings(seen_at_test[0], seen_at_test[1]), test_users)
    print(f"test {fmt(metrics(model, test_users, test_targets, test_seen))}")


if __name__ == "__main__":
    main()
