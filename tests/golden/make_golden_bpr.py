"""Generate the pair-wise (BPR) golden vectors g9_* under tests/golden/ by running the REFERENCE itself on CPU.

    python tests/golden/make_golden_bpr.py <reference checkout>        (or set NCF_REFERENCE_DIR)

g9_bpr_sampling   schedule_w(1..30) (train.py:229-243); RankingDataset._negative_sampling_probs (datasets/base.py:57-70) for every
                  type and every scheduled w on rows of mixed lengths with repeated ratings (and a zero rating); the reference's
                  RankingDataset.__getitem__ (:72-78) draws for every row under np.random.seed (the dataset is built with __new__
                  and given ``samples``: its __init__ reads HDF5); BPR_loss (:97-98) on given pairs, and on pairs one of which is
                  past fp32's sigmoid underflow (the loss is inf).
g9_bpr_basic / g9_bpr_mf / g9_bpr_att   the reference model in .train() with dropout 0 / None, (user, positive, negative) triplets
                  through the reference's ranking do_forward (fixed_datasets.py:50-57 on one-hot rows, dynamic_datasets.py:54-61):
                  out_pos, out_neg, the BPR loss, every parameter gradient and the magnitude of the two calls' shares of it.
                  AttentionNCF's candidates are rated rows of the batch (as the ranking file's positives and negatives are), so the
                  train-mode target mask (attention_ncf.py:195-205) acts.

Lists are stored as CSR arrays (rowptr + concatenated values): load_golden refuses pickles.  The helpers (reference import with its
stub modules, state arrays, writer) are make_golden.py's.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

W_SCHEDULE = (0.0, 0.5, 1, 1.5, 3)
PROB_TYPES = ("sum", "sum_dynamic", "softmax")
DRAW_ROUNDS = 25


def sampling_rows():
    rng = np.random.default_rng(91)
    ids, ratings = [], []
    for n in (1, 2, 3, 7, 17, 64, 65, 300):
        ids.append(rng.choice(np.arange(1000, 5000), size=n, replace=False).astype(np.int64))
        ratings.append((rng.integers(1, 10, n) * 0.5).astype(np.float64))      # 0.5 .. 4.5: repeated values
    ratings[3][2] = 0.0            # a zero rating inside a row
    ratings[4][0] = 0.0            # and one at a row's start
    return ids, ratings


def golden_sampling(torch):
    import pandas as pd
    from neural_collaborative_filtering.datasets.base import BPR_loss, RankingDataset
    from neural_collaborative_filtering.train import schedule_w
    ids, ratings = sampling_rows()
    out = {"schedule_w": np.array([schedule_w(e) for e in range(1, 31)], dtype=np.float64),
           "rowptr": np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int64),
           "neg_ids": np.concatenate(ids), "neg_ratings": np.concatenate(ratings), "w_values": np.array(W_SCHEDULE, dtype=np.float64),
           "draw_rounds": np.array(DRAW_ROUNDS)}
    ds = RankingDataset.__new__(RankingDataset)
    ds.samples = pd.DataFrame({"userId": np.arange(len(ids)) + 1, "positive_movieId": np.arange(len(ids)) + 9000,
                               "negative_movieIds": [list(x) for x in ids], "negative_ratings": [list(x) for x in ratings]})
    for k, w in enumerate(W_SCHEDULE):
        ds.w = w
        for t in PROB_TYPES:
            out[f"probs_{t}_{k}"] = np.concatenate([np.asarray(ds._negative_sampling_probs(np.array(r), type=t), dtype=np.float64)
                                                    for r in ratings])
        assert all(ds._negative_sampling_probs(np.array(r), type="uniform") is None for r in ratings)
        np.random.seed(1234 + k)
        out[f"draws_{k}"] = np.array([ds[i][2] for _ in range(DRAW_ROUNDS) for i in range(len(ids))], dtype=np.int64)
    g = torch.Generator().manual_seed(5)
    pos, neg = torch.randn(64, 1, generator=g) * 3, torch.randn(64, 1, generator=g) * 3
    pos_u, neg_u = pos.clone(), neg.clone()
    pos_u[5, 0], neg_u[5, 0] = -60.0, 60.0      # sigmoid(-120) is 0 in fp32: -log(0) = inf
    loss, loss_u = BPR_loss(pos, neg).item(), BPR_loss(pos_u, neg_u).item()
    assert np.isfinite(loss) and np.isinf(loss_u)
    out.update(bpr_pos=pos.numpy(), bpr_neg=neg.numpy(), bpr_loss=np.array(loss),
               bpr_pos_under=pos_u.numpy(), bpr_neg_under=neg_u.numpy(), bpr_loss_under=np.array(loss_u))
    G._save("g9_bpr_sampling", **out)


def _onehot(torch, pos, n):
    x = torch.zeros((len(pos), n), dtype=torch.float32)
    x[torch.arange(len(pos)), torch.as_tensor(pos)] = 1.0
    return x


def _grads(m, out_pos, out_neg, loss):
    """Every parameter gradient of the loss (``g::``), and per element the sum of the magnitudes of the two calls' shares of it
    (``s::`` = |d loss / d out_pos . d out_pos / d p| + |the same through out_neg|): BPR's gradient is a difference of the two
    shares, so its fp32 rounding scales with them, not with the (cancelled) result."""
    import torch
    params = [p for _, p in m.named_parameters()]
    d_pos, d_neg = torch.autograd.grad(loss, (out_pos, out_neg), retain_graph=True)
    share_pos = torch.autograd.grad(out_pos, params, grad_outputs=d_pos, retain_graph=True, allow_unused=True)
    share_neg = torch.autograd.grad(out_neg, params, grad_outputs=d_neg, retain_graph=True, allow_unused=True)
    loss.backward()
    grads = {"g::" + k: p.grad.detach().numpy().copy() for k, p in m.named_parameters()}
    assert all(np.isfinite(v).all() for v in grads.values())
    for (k, _), a, b in zip(m.named_parameters(), share_pos, share_neg):
        grads["s::" + k] = sum(t.detach().abs() for t in (a, b) if t is not None).numpy()
    return grads


def golden_fixed(torch, tag, m, U, I, B, seed):
    from neural_collaborative_filtering.datasets.base import BPR_loss
    from neural_collaborative_filtering.datasets.fixed_datasets import FixedRankingDataset
    rng = np.random.default_rng(seed)
    up, pp, npos = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    batch = (_onehot(torch, up, U), _onehot(torch, pp, I), _onehot(torch, npos, I))
    out_pos, out_neg = FixedRankingDataset.do_forward(m, batch, torch.device("cpu"))
    loss = BPR_loss(out_pos, out_neg)
    grads = _grads(m, out_pos, out_neg, loss)
    G._save(tag, user_pos=up, pos_pos=pp, neg_pos=npos, out_pos=out_pos.detach().numpy(), out_neg=out_neg.detach().numpy(),
            loss=np.array(loss.item()), kwargs=np.array(json.dumps(m.kwargs)), **G._state_arrays(m), **grads)


def golden_att(torch, AttentionNCF):
    from neural_collaborative_filtering.datasets.base import BPR_loss
    from neural_collaborative_filtering.datasets.dynamic_datasets import DynamicRankingDataset
    torch.manual_seed(403)
    Fdim, B, I = 20, 12, 15
    m = AttentionNCF(item_dim=Fdim, item_emb=16, user_emb=16, att_dense=8, mlp_dense_layers=[32, 16], dropout_rate=0.0,
                     message_dropout=None).train()
    g = torch.Generator().manual_seed(404)
    rated = torch.rand(I, Fdim, generator=g)
    um = torch.zeros(B, I)
    mask = torch.rand(B, I, generator=g) < 0.6
    um[mask] = (torch.randint(1, 11, (B, I), generator=g).float() * 0.5 - 2.9)[mask]
    cand1, cand2 = torch.rand(B, Fdim, generator=g), torch.rand(B, Fdim, generator=g)
    pos_col, neg_col = np.full(B, -1), np.full(B, -1)
    for b in range(B - 2):                       # the last two rows: candidates that are no rated row (nothing to mask)
        cols = torch.randperm(I, generator=g)[:2].tolist()
        pos_col[b], neg_col[b] = cols
        um[b, cols[0]], um[b, cols[1]] = 1.6, -0.4      # the user rated both, the positive higher
        cand1[b], cand2[b] = rated[cols[0]], rated[cols[1]]
    batch = (None, None, cand1, rated, um, cand2)
    out_pos, out_neg = DynamicRankingDataset.do_forward(m, batch, torch.device("cpu"))
    loss = BPR_loss(out_pos, out_neg)
    grads = _grads(m, out_pos, out_neg, loss)
    G._save("g9_bpr_att", candidate_items1=cand1.numpy(), candidate_items2=cand2.numpy(), rated_items=rated.numpy(), user_matrix=um.numpy(),
            pos_col=pos_col, neg_col=neg_col, out_pos=out_pos.detach().numpy(), out_neg=out_neg.detach().numpy(), loss=np.array(loss.item()),
            kwargs=np.array(json.dumps(m.kwargs)), **G._state_arrays(m), **grads)


def main():
    G._import_reference()
    import torch
    from neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    from neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from neural_collaborative_filtering.models.mf import MF
    torch.set_num_threads(1)
    golden_sampling(torch)
    torch.manual_seed(401)
    U, I = 120, 80
    golden_fixed(torch, "g9_bpr_basic", BasicNCF(item_dim=I, user_dim=U, item_emb=32, user_emb=32, mlp_dense_layers=[64, 32],
                                                 dropout_rate=None).train(), U, I, 160, 41)
    torch.manual_seed(402)
    golden_fixed(torch, "g9_bpr_mf", MF(item_dim=40, user_dim=60, item_emb=16, user_emb=16).train(), 60, 40, 96, 42)
    golden_att(torch, AttentionNCF)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        G.REF = args[0]
    if not G.REF or not os.path.isdir(os.path.join(G.REF, "src")):
        raise SystemExit("usage: make_golden_bpr.py <reference checkout>  (or set NCF_REFERENCE_DIR)")
    main()
