"""Generate tests/golden/g9_att_stats.npz by running the REFERENCE itself on CPU: the item-item attention statistics its
evaluation loop accumulates over a test file (eval.py:101-108, 137-143), on a small AttentionNCF.

    python tests/golden/make_att_stats_golden.py <reference checkout>          (or set NCF_REFERENCE_DIR)

The reference's model is imported the way make_golden.py does it.  The fixture holds data only: the weights (``w::`` entries), the
constructor kwargs, the catalogue's features, the users' CSR (rows = users, columns = catalogue positions, ascending), the sample
file (user row and candidate position per sample) and the reference's two tables."""
import json
import os
import sys

import numpy as np

import make_golden as G

N_ITEMS, F_DIM, N_USERS, N_SAMPLES, BATCH = 48, 20, 24, 160, 32
ATT_GAIN = 24.0                      # AttentionNet's last Linear scaled so that the softmax is not flat
ROW_LENS = (0, 1, 2, 3, 5, 8, 13, 21, 33, 34, 40, 48)     # the first users' rated items: none, one, more than 32, all


def main():
    G._import_reference()
    import torch
    from neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.set_num_threads(1)
    torch.manual_seed(901)
    m = AttentionNCF(item_dim=F_DIM, item_emb=16, user_emb=16, att_dense=8, mlp_dense_layers=[32, 16]).eval()
    with torch.no_grad():
        m.AttentionNet[-1].weight.mul_(ATT_GAIN)
    rng = np.random.default_rng(902)
    g = torch.Generator().manual_seed(903)
    features = torch.rand(N_ITEMS, F_DIM, generator=g)
    lens = list(ROW_LENS) + rng.integers(0, N_ITEMS + 1, N_USERS - len(ROW_LENS)).tolist()
    rowptr = np.zeros(N_USERS + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.permutation(N_ITEMS)[:n]) for n in lens]).astype(np.int32)
    val = (rng.integers(1, 11, len(col)) * 0.5 - 2.9).astype(np.float32)          # -2.4 .. 2.1, never 0
    dense = np.zeros((N_USERS, N_ITEMS), dtype=np.float32)
    for u in range(N_USERS):
        dense[u, col[rowptr[u]:rowptr[u + 1]]] = val[rowptr[u]:rowptr[u + 1]]
    # the sample file: every user occurs, a third of the catalogue is never a candidate, one candidate takes a quarter of the samples
    users = np.concatenate([np.arange(N_USERS), rng.integers(0, N_USERS, N_SAMPLES - N_USERS)])
    pool = np.array([c for c in range(N_ITEMS) if c % 3 != 1])
    cands = rng.choice(pool, N_SAMPLES)
    cands[rng.permutation(N_SAMPLES)[:N_SAMPLES // 4]] = 7
    p = rng.permutation(N_SAMPLES)
    users, cands = users[p].astype(np.int64), cands[p].astype(np.int64)

    # eval.py:101-108: the whole catalogue is the rated list, so rated_pos = 0 .. n - 1
    n = N_ITEMS
    att_stats = {'sum': np.zeros((n, n)), 'count': np.zeros((n, n), dtype=np.int64)}
    rated_pos = np.arange(n)
    with torch.no_grad():
        for s in range(0, N_SAMPLES, BATCH):
            candidate_pos = cands[s:s + BATCH]
            user_matrix = torch.from_numpy(dense[users[s:s + BATCH]])
            _, att_weights = m(features[torch.from_numpy(candidate_pos)], features, user_matrix, return_attention_weights=True)
            att_weights = att_weights.cpu().numpy()
            user_matrix = user_matrix.cpu().numpy()
            counts = np.array(np.logical_or(user_matrix != 0.0, att_weights > 0.0), dtype=np.int64)      # eval.py:140
            for i, c in enumerate(candidate_pos):                                                          # eval.py:141-143
                att_stats['sum'][c, rated_pos] += att_weights[i, :]
                att_stats['count'][c, rated_pos] += counts[i, :]
    mean_w = att_stats['sum'][att_stats['count'] > 0] / att_stats['count'][att_stats['count'] > 0]
    print("cells with a count:", int((att_stats['count'] > 0).sum()), "mean weight per cell: min %.3g max %.3g" % (mean_w.min(), mean_w.max()))
    assert mean_w.max() > 10 * np.median(mean_w)                                          # the softmax is not flat
    G._save("g9_att_stats", features=features.numpy(), rowptr=rowptr, col=col, val=val, users=users, cands=cands,
            sum=att_stats['sum'], count=att_stats['count'], att_gain=np.array(ATT_GAIN), kwargs=np.array(json.dumps(m.kwargs)),
            **G._state_arrays(m))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        G.REF = args[0]
    if not G.REF or not os.path.isdir(os.path.join(G.REF, "src")):
        raise SystemExit("usage: make_att_stats_golden.py <reference checkout>  (or set NCF_REFERENCE_DIR)")
    main()
