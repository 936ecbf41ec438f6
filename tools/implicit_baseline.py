"""The implicit-feedback baseline of a full-catalogue ranking evaluation on the device: ImplicitALS chosen by validation NDCG@10.

    python tools/implicit_baseline.py TRAIN VAL TEST [--factors 32 64 128] [--regs 0.01 0.1] [--alphas 10 40] [--iters 15]
                                                     [--min-rating 0] [--seed 0]

TRAIN / VAL / TEST are the sample files (CSV with userId, movieId, rating columns; ``.csv`` may be left off).  Every rating of at
least ``--min-rating`` is an interaction, held with confidence 1 + alpha * rating; a pair listed twice keeps its last rating.  Grid
search over factors x reg x alpha: every grid point is fitted on TRAIN and prints the full-catalogue HR@10, NDCG@10, MRR and AUC of
VAL's items (``eval_full_ranking`` on ``as_mf()``, every item of the catalogue ranked, the user's TRAIN items left out).  The grid
point with the best validation NDCG@10 is then scored on TEST the same way, with the TRAIN and the VAL items left out.  Users of VAL /
TEST without a TRAIN interaction are scored from a zero vector, as any model without a row for them would."""
import argparse
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import ImplicitALS, eval_full_ranking, held_out_items, rated_exclusion  # noqa: E402
from deeprecommendation_amd.baselines import build_csr  # noqa: E402


def read_samples(path):
    path = path if os.path.exists(path) else path + ".csv"
    return pd.read_csv(path, usecols=["userId", "movieId", "rating"])


class Ratings:
    """The two arrays rated_exclusion reads."""

    def __init__(self, rowptr, col):
        self.rowptr, self.col = rowptr, col


def csr_of(frames, lookup_u, lookup_i, n_users, n_items, min_rating, dev):
    """One CSR over the interactions of ``frames``: what a user holds, hence what is left out of their ranked list."""
    f = pd.concat(frames).drop_duplicates(["userId", "movieId"], keep="last")
    f = f[f["rating"] >= min_rating]
    u = torch.from_numpy(lookup_u.loc[f["userId"]].to_numpy()).to(dev)
    i = torch.from_numpy(lookup_i.loc[f["movieId"]].to_numpy()).to(dev)
    return build_csr(u, i, torch.from_numpy(f["rating"].to_numpy(dtype=np.float32)).to(dev), n_users, n_items)


def fmt(m):
    return f"HR@10 {m['hr@10']:.4f}, NDCG@10 {m['ndcg@10']:.4f}, MRR {m['mrr']:.4f}, AUC {m['auc']:.4f} ({int(m['users'])} users)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("train"), ap.add_argument("val"), ap.add_argument("test")
    ap.add_argument("--factors", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--regs", type=float, nargs="+", default=[0.01, 0.1])
    ap.add_argument("--alphas", type=float, nargs="+", default=[10.0, 40.0])
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--min-rating", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
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

    val_users, val_targets = held(frames[1])
    test_users, test_targets = held(frames[2])
    val_seen = rated_exclusion(Ratings(train[0], train[1]), val_users)
    best = None
    for factors in args.factors:
        for reg in args.regs:
            for alpha in args.alphas:
                model = ImplicitALS(n_factors=factors, n_iters=args.iters, reg=reg, alpha=alpha)
                model.fit_csr(*train, n_items, generator=torch.Generator().manual_seed(args.seed))
                m = eval_full_ranking(model.as_mf(), val_users, val_targets, exclude=val_seen, cutoffs=(10,))
                print(f"factors={factors} reg={reg} alpha={alpha} iters={args.iters}: val {fmt(m)}", flush=True)
                if best is None or m["ndcg@10"] > best[0]["ndcg@10"]:
                    best = (m, model)
    m, model = best
    print(f"best by val NDCG@10: factors={model.n_factors} reg={model.reg} alpha={model.alpha} (val NDCG@10 {m['ndcg@10']:.4f})")
    test_seen = rated_exclusion(Ratings(seen_at_test[0], seen_at_test[1]), test_users)
    print(f"test {fmt(eval_full_ranking(model.as_mf(), test_users, test_targets, exclude=test_seen, cutoffs=(10,)))}")


if __name__ == "__main__":
    main()
