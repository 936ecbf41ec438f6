"""GPU: top_k_items (BasicNCF / MF) and recommend_for_user (AttentionNCF) against CPU oracles.

Scores are held to the parity bar |a - b| <= 1e-5 |b| + 1e-6 max|b| (test_gpu_basic.py).  Ranks: sorting is 1-Lipschitz, so the
k-th best score of the device and of the oracle are within the bar of each other at every rank; ids must be equal at every rank
whose oracle score is separated from both neighbours by more than twice the bar (elsewhere fp32 rounding may legitimately swap two
near-equal items)."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from oracle import ncf_oracle as O
from test_topk_cpu import topk_oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-5


def _bar(ref, scale):
    return RTOL * np.abs(ref) + 0.1 * RTOL * scale


def _model(cls, kw, state, gpu):
    m = cls(**kw)
    m.load_state_dict(state)
    return m.eval().to(gpu)


def _check_ranked(got_s, got_id, got_n, ref_s, ref_id, ref_n, scale):
    """One ranked list against the oracle's (numpy 1-D arrays of the valid entries' scores / ids)."""
    assert got_n == ref_n
    got_s, got_id, ref_s, ref_id = got_s[:got_n], got_id[:got_n], ref_s[:ref_n], ref_id[:ref_n]
    bar = _bar(ref_s, scale)
    assert np.all(np.abs(got_s - ref_s) <= bar), np.max(np.abs(got_s - ref_s) - bar)
    ext = np.concatenate([[np.inf], ref_s, [-np.inf]])
    isolated = (ext[:-2] - ext[1:-1] > 2 * bar) & (ext[1:-1] - ext[2:] > 2 * bar)
    assert np.array_equal(got_id[isolated], ref_id[isolated])


# ---------------------------------------------------------------------------------------- top_k_items
def _all_pairs_oracle(forward, state, users, n_items):
    u = torch.as_tensor(users).repeat_interleave(n_items)
    i = torch.arange(n_items).repeat(len(users))
    return forward(state, u, i).view(len(users), n_items)


@pytest.mark.parametrize("name,k,with_exclude,block_bytes", [
    ("g1_basic_onehot_e64", 10, False, None), ("g1_basic_onehot_e64", 100, True, None),
    ("g1_basic_onehot_e64", 50, True, 64 * 400 * 20),            # 64 users per score block: five blocks
    ("g2_mf_onehot", 5, False, None), ("g2_mf_onehot", 40, True, 7 * 40 * 20)])
def test_top_k_items_matches_oracle(gpu, name, k, with_exclude, block_bytes):
    from deeprecommendation_amd import top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    state, a, kw = load_golden(name)
    basic = name.startswith("g1")
    m = _model(BasicNCF if basic else MF, kw, state, gpu)
    U, I = kw["user_dim"], kw["item_dim"]
    rng = np.random.default_rng(len(name) + k)
    users = rng.integers(0, U, 300 if basic else 50)
    ref = _all_pairs_oracle(O.basic_ncf_forward_indexed if basic else O.mf_forward_indexed, state, users, I)
    lists = [rng.integers(0, I, int(rng.integers(0, I // 2))).tolist() for _ in users] if with_exclude else None
    exclude = None
    if with_exclude:
        lists[0] = list(range(I))                                  # a user who has rated everything: count 0
        rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=gpu)
        col = torch.tensor(np.concatenate([np.asarray(x, np.int64) for x in lists]), dtype=torch.int32, device=gpu)
        exclude = (rowptr, col)
    kwargs = {} if block_bytes is None else {"block_bytes": block_bytes}
    s, pos, n = top_k_items(m, torch.as_tensor(users, device=gpu), k, exclude=exclude, **kwargs)
    assert s.shape == (len(users), k) and pos.dtype == torch.int64
    rs, ri, rn = topk_oracle(ref, k, lists)
    s, pos, n = s.cpu().numpy(), pos.cpu().numpy(), n.cpu().numpy()
    scale = float(ref.abs().max())
    for r in range(len(users)):
        _check_ranked(s[r], pos[r], int(n[r]), rs[r].numpy(), ri[r].numpy(), int(rn[r]), scale)
        assert np.all(pos[r, n[r]:] == -1) and np.all(np.isneginf(s[r, n[r]:]))


def test_top_k_items_item_subset(gpu):
    from deeprecommendation_amd import top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    state, a, kw = load_golden("g1_basic_onehot_e64")
    m = _model(BasicNCF, kw, state, gpu)
    items = np.arange(3, kw["item_dim"], 7)
    users = np.array([0, 5, 599])
    ref = O.basic_ncf_forward_indexed(state, torch.as_tensor(users).repeat_interleave(len(items)),
                                      torch.as_tensor(items).repeat(len(users))).view(len(users), len(items))
    s, pos, n = top_k_items(m, torch.as_tensor(users, device=gpu), 20, item_ids=torch.as_tensor(items, device=gpu))
    rs, ri, rn = topk_oracle(ref, 20)
    for r in range(len(users)):
        _check_ranked(s[r].cpu().numpy(), pos[r].cpu().numpy(), int(n[r]), rs[r].numpy(), items[ri[r].numpy()], int(rn[r]),
                      float(ref.abs().max()))


# ---------------------------------------------------------------------------------------- recommend_for_user
def reference_recommend_for_user(state, kw, item_features, user_ratings, k, ignore_seen, explain_factor=1.5, explain_constant=0.025):
    """CPU restatement of the reference's webapp/backend.py:78-121 over the oracle forward (ncf_oracle.attention_ncf_forward).
    Differences, both deliberate: the final sort is stable (the reference's default quicksort leaves equal scores in an
    unspecified order), and every winner's full weight row is returned next to the frame for the weight comparison."""
    items_to_use = item_features.drop(user_ratings.index) if ignore_seen else item_features                      # :84
    candidate_items = torch.FloatTensor(items_to_use.values)                                                      # :85
    rated_items_ids = np.sort(np.unique(user_ratings.index))                                                       # :88
    rated_items = torch.FloatTensor(item_features.loc[rated_items_ids].values)                                     # :89
    user_matrix = torch.FloatTensor(np.repeat(np.expand_dims(user_ratings.loc[rated_items_ids].values                  # :92
                                                             - ((user_ratings.mean() + 2.5) / 2), axis=0),
                                              candidate_items.shape[0], axis=0))
    y_pred, att_weights = O.attention_ncf_forward(state, candidate_items, rated_items, user_matrix,              # :94-98
                                                  use_cos_sim_instead=kw["use_cos_sim_instead"], return_attention_weights=True)
    y_pred = y_pred.view(-1).numpy()
    att_weights = att_weights.numpy()
    exp_thr = explain_factor * (1 / max(len(rated_items_ids), 1)) + explain_constant                             # :105
    mask = att_weights > exp_thr                                                                                  # :106
    exp = [rated_items_ids[m] for m in mask]                                                                       # :109
    att = [att_weights[i, m] for i, m in enumerate(mask)]                                                         # :110
    predictions = pd.DataFrame(data={'imdbID': items_to_use.index, 'score': y_pred, 'because': exp, 'attention': att})   # :113-118
    order = predictions.sort_values(by='score', ascending=False, kind='stable').index[:k]
    return predictions.loc[order], att_weights[np.asarray(order)], exp_thr, float(np.abs(y_pred).max())


def _catalogue(n_items, n_feat, seed):
    rng = np.random.default_rng(seed)
    feats = (rng.random((n_items, n_feat)) < 0.15).astype(np.float32) * rng.random((n_items, n_feat)).astype(np.float32)
    return pd.DataFrame(feats, index=[f"tt{1000000 + 37 * i:07d}" for i in range(n_items)])


def _ratings(cat, n, seed):
    rng = np.random.default_rng(seed)
    ids = rng.choice(cat.index.to_numpy(), n, replace=False)
    vals = rng.integers(1, 11, n) * 0.5
    return pd.Series(index=ids, data=vals, dtype=float)


def _compare_recommendations(got, ref, ref_att_rows, rated_ids, exp_thr, catalogue_scores_scale):
    assert list(got.columns) == ['imdbID', 'score', 'because', 'attention']
    assert len(got) == len(ref)
    _check_ranked(got['score'].to_numpy(np.float32), got['imdbID'].to_numpy(), len(got), ref['score'].to_numpy(np.float32),
                  ref['imdbID'].to_numpy(), len(ref), catalogue_scores_scale)
    ref_by_id = {iid: j for j, iid in enumerate(ref['imdbID'])}
    att_scale = float(np.abs(ref_att_rows).max()) if ref_att_rows.size else 0.0
    for _, row in got.iterrows():
        j = ref_by_id.get(row['imdbID'])
        if j is None:                      # a near-tie swapped in at the cut: its rank was already held to the bar above
            continue
        w = ref_att_rows[j]
        g_because, g_att = list(row['because']), np.asarray(row['attention'])
        r_because = list(ref.iloc[j]['because'])
        # weights of the items the device reports, against the oracle's weights of the same rated items
        ref_w = w[np.searchsorted(rated_ids, g_because)] if g_because else np.zeros(0)
        assert np.all(np.abs(g_att - ref_w) <= _bar(ref_w, att_scale))
        # the two 'because' lists agree except for items whose oracle weight is within the bar of the threshold
        for iid in set(g_because) ^ set(r_because):
            wi = w[np.searchsorted(rated_ids, iid)]
            assert abs(wi - exp_thr) <= _bar(np.float32(exp_thr), att_scale), (iid, wi, exp_thr)


@pytest.mark.parametrize("name", ["g3_att_vec64", "g3_att_dense8"])
@pytest.mark.parametrize("ignore_seen", [True, False])
@pytest.mark.parametrize("n_items,n_rated,k", [(3000, 40, 10), (3000, 60, 100), (120, 30, 200)])    # last: k > unseen items
def test_recommend_for_user_matches_reference(gpu, name, ignore_seen, n_items, n_rated, k):
    from deeprecommendation_amd import recommend_for_user
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    state, _, kw = load_golden(name)
    m = _model(AttentionNCF, kw, state, gpu)
    cat = _catalogue(n_items, kw["item_dim"], n_items + n_rated)
    ratings = _ratings(cat, n_rated, k)
    got = recommend_for_user(m, cat, ratings, k=k, ignore_seen=ignore_seen)
    ref, ref_att, thr, scale = reference_recommend_for_user(state, kw, cat, ratings, k, ignore_seen)
    if k > n_items - n_rated and ignore_seen:
        assert len(got) == n_items - n_rated
    assert not ignore_seen or not set(got['imdbID']) & set(ratings.index)
    _compare_recommendations(got, ref, ref_att, np.sort(np.unique(ratings.index)), thr, scale)


def test_recommend_for_user_repeated_request_reuses_catalogue(gpu):
    """Second request with the same DataFrame: the identical frame, the same catalogue tensor, and the model's kept candidate
    projections (the 'candidates' cache entry) are hit, not rebuilt — the winners' rerun does not displace them."""
    from deeprecommendation_amd import recommend as rec
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    state, _, kw = load_golden("g3_att_vec64")
    m = _model(AttentionNCF, kw, state, gpu)
    cat = _catalogue(2000, kw["item_dim"], 77)
    ratings = _ratings(cat, 50, 78)
    first = rec.recommend_for_user(m, cat, ratings, k=25)
    kept = m._native_cache["candidates"]
    feats = rec._catalogue_cache[torch.device(gpu)][1]
    assert kept[3] is feats                                          # the projections kept are those of the catalogue tensor
    second = rec.recommend_for_user(m, cat, ratings, k=25)
    assert m._native_cache["candidates"] is kept                     # a hit leaves the entry as it was; a miss replaces it
    assert rec._catalogue_cache[torch.device(gpu)][1] is feats
    assert first['imdbID'].tolist() == second['imdbID'].tolist()
    assert np.array_equal(first['score'].to_numpy(), second['score'].to_numpy())
    assert first.index.tolist() == second.index.tolist()
    for a, b in zip(first['attention'], second['attention']):
        assert np.array_equal(a, b)
    for a, b in zip(first['because'], second['because']):
        assert list(a) == list(b)
    ref, ref_att, thr, scale = reference_recommend_for_user(state, kw, cat, ratings, 25, True)
    _compare_recommendations(second, ref, ref_att, np.sort(np.unique(ratings.index)), thr, scale)


def test_recommend_for_user_accepts_a_device_catalogue(gpu):
    from deeprecommendation_amd import recommend_for_user
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    state, _, kw = load_golden("g3_att_vec64")
    m = _model(AttentionNCF, kw, state, gpu)
    cat = _catalogue(500, kw["item_dim"], 5)
    ratings = _ratings(cat, 20, 6)
    a = recommend_for_user(m, cat, ratings, k=30)
    b = recommend_for_user(m, (torch.from_numpy(cat.values).to(gpu), cat.index.to_numpy()), ratings, k=30)
    assert a['imdbID'].tolist() == b['imdbID'].tolist()
    assert np.array_equal(a['score'].to_numpy(), b['score'].to_numpy())
