"""GPU tests of the ItemKNN baseline, bit for bit against the fp32 restatement of tests/knn_ref.py: squared norms, similarity rows over
three column tiles (forced and default), the neighbour table through ncf_topk_rows (exact ties included), scores on the staged and
the unstaged path from a CSR other than the fitted one, predict == scores, the ranking front ends against a numpy sort, the two
sticky flags on inputs the kernel must refuse by checking, blocking and repeatability."""
import numpy as np
import pytest
import torch

import knn_ref as K

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(arrays, gpu):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays)


def _fit(gpu, case, n_items, N, shrink, min_support, **kw):
    import deeprecommendation_amd as pkg
    rowptr, col, val = _dev(case, gpu)
    model_args = {k: kw.pop(k) for k in ("weighted_average", "fill") if k in kw}
    return pkg.ItemKNN(k=N, shrink=shrink, min_support=min_support, **model_args).fit_csr(rowptr, col, val, n_items, **kw)


def _table_same(model, table):
    pos, sim, cnt = table
    return _same(model.nb_pos_, pos) and _same(model.nb_sim_, sim) and _same(model.nb_cnt_, cnt)


def test_item_sq_matches_the_lane_partials_and_the_tree(gpu):
    from deeprecommendation_amd import native
    colptr, row, tval = K.transpose_ref(*K.base_case(), K.I)
    assert np.diff(colptr).max() > 64                                  # a lane takes a second step
    d = _dev((colptr, tval), gpu)
    assert _same(native.knn_item_sq(*d), K.base_gram()[2])
    native.check_oob(gpu)


@pytest.mark.parametrize("col_tile", [64, 0])
@pytest.mark.parametrize("shrink,min_support", K.SIM_PARAMS)
def test_sim_rows_match_the_restatement_bit_for_bit(gpu, col_tile, shrink, min_support):
    from deeprecommendation_amd import native
    csr = K.base_case()
    d = _dev(csr + K.transpose_ref(*csr, K.I), gpu)
    sq = native.knn_item_sq(d[3], d[5])
    want = K.base_sim(shrink, min_support)
    got = native.knn_sim_rows(*d, sq, None, min_support, shrink, col_tile)
    assert _same(got, want)
    assert not want[K.UNRATED_ITEM].any() and not want[:, K.UNRATED_ITEM].any() and (want[K.COMMON_ITEM] > 0).sum() > 20
    part = native.knn_sim_rows(*d, sq, (60, 131), min_support, shrink, col_tile)       # a block of rows that starts mid-tile
    assert _same(part, want[60:131])
    native.check_oob(gpu), native.check_knn(gpu)


@pytest.mark.parametrize("N,shrink,min_support,col_tile", [(1, 0.0, 1, 64), (7, 10.0, 2, 64), (200, 0.0, 1, 0), (7, 0.0, 1, 0),
                                                           (200, 10.0, 2, 64)])
def test_fit_gives_the_reference_table(gpu, N, shrink, min_support, col_tile):
    m = _fit(gpu, K.base_case(), K.I, N, shrink, min_support, col_tile=col_tile)
    want = K.base_table(N, shrink, min_support)
    assert _table_same(m, want)
    assert want[2].max() <= min(N, 148) and want[2][K.UNRATED_ITEM] == 0
    sim, pos, cnt = m.neighbours
    assert pos.dtype == torch.int64 and np.array_equal(pos.cpu().numpy(), want[0].astype(np.int64)) and sim is m.nb_sim_
    items = torch.tensor([K.COMMON_ITEM, K.UNRATED_ITEM, 149], device=gpu)
    k = min(N, 3)
    s, p, c = m.similar_items(items, k)
    assert np.array_equal(p.cpu().numpy(), want[0][[K.COMMON_ITEM, K.UNRATED_ITEM, 149], :k].astype(np.int64))
    assert np.array_equal(c.cpu().numpy(), np.minimum(want[2][[K.COMMON_ITEM, K.UNRATED_ITEM, 149]], k))
    assert torch.isinf(s[1]).all() and (p[1] == -1).all() and _same(s[0], want[1][K.COMMON_ITEM, :k])


def test_exact_ties_go_to_the_lower_position_and_a_fit_repeats_its_bits(gpu):
    case = K.integer_case()
    S = K.sim_ref(*case, 70, 0.0, 1)
    want = K.table_ref(S, 7)
    tied = sum(int((want[1][i, :-1] == want[1][i, 1:]).sum()) for i in range(70) if want[2][i] == 7)
    assert tied > 20                                                   # the rule decides slots of the kept table, not only its tail
    a = _fit(gpu, case, 70, 7, 0.0, 1, col_tile=64)
    assert _table_same(a, want)
    b = _fit(gpu, case, 70, 7, 0.0, 1, col_tile=64)                    # the same fit once more: the same bits
    assert _same(b.nb_pos_, a.nb_pos_.cpu().numpy()) and _same(b.nb_sim_, a.nb_sim_.cpu().numpy()) and _same(b.nb_cnt_, a.nb_cnt_.cpu().numpy())
    assert _table_same(_fit(gpu, case, 70, 7, 0.0, 1), want)           # one tile of 128 columns


def test_a_fit_in_two_item_blocks_gives_the_bits_of_one(gpu):
    want = K.base_table(7, 10.0, 1)
    one = _fit(gpu, K.base_case(), K.I, 7, 10.0, 1)
    two = _fit(gpu, K.base_case(), K.I, 7, 10.0, 1, block_bytes=4 * K.I * 80)      # rows [0, 80) and [80, 150)
    assert _table_same(one, want) and _table_same(two, want)


def test_fit_from_samples_in_any_order(gpu):
    import deeprecommendation_amd as pkg
    rowptr, col, val = K.base_case()
    us = np.repeat(np.arange(K.U), np.diff(rowptr))
    perm = np.random.default_rng(5).permutation(len(us))
    u, i, r = _dev((us[perm], col.astype(np.int64)[perm], val[perm]), gpu)
    m = pkg.ItemKNN(k=7, shrink=10.0, min_support=2).fit(u, i, r, K.U, K.I)
    assert _table_same(m, K.base_table(7, 10.0, 2))


def test_fit_dataset_is_the_fit_on_the_providers_positions(gpu):
    import pandas as pd
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset
    rowptr, col, val = K.base_case()
    us = np.repeat(np.arange(K.U), np.diff(rowptr))
    perm = np.random.default_rng(6).permutation(len(us))
    train = pd.DataFrame({"userId": us[perm] * 3 + 30, "movieId": col[perm].astype(np.int64) * 7 + 7, "rating": val[perm].astype(np.float64)})
    cp = IndexProvider(np.arange(K.U) * 3 + 30, np.arange(K.I) * 7 + 7)
    a = pkg.ItemKNN(k=7, shrink=10.0, min_support=2).fit_dataset(FixedPointwiseDataset(train, cp), gpu)
    u, i, r = _dev((us[perm], col[perm].astype(np.int64), val[perm]), gpu)
    b = pkg.ItemKNN(k=7, shrink=10.0, min_support=2).fit(u, i, r, K.U, K.I)
    assert torch.equal(a.nb_pos_, b.nb_pos_) and torch.equal(a.nb_sim_, b.nb_sim_) and torch.equal(a.nb_cnt_, b.nb_cnt_)
    assert _table_same(a, K.base_table(7, 10.0, 2))


@pytest.mark.parametrize("stage_cap", [64, 0])
@pytest.mark.parametrize("weighted,fill", [(True, -3.5), (False, 0.0)])
def test_scores_of_new_users_on_both_paths_and_predict(gpu, stage_cap, weighted, fill):
    m = _fit(gpu, K.base_case(), K.I, 7, 10.0, 2, weighted_average=weighted, fill=fill)
    ratings = _dev(K.score_case(), gpu)
    B = len(K.score_case()[0]) - 1
    users = torch.arange(B, device=gpu)
    want = K.base_scores(7, 10.0, 2, weighted, fill)
    got = m.scores(ratings, users, stage_cap=stage_cap)
    assert _same(got, want)
    if weighted:                                                       # den = 0: an empty row, a row without any neighbour, nobody's item
        assert (want[1] == fill).all() and (want[3] == fill).all() and (want[:, K.UNRATED_ITEM] == fill).all()
    some = torch.tensor([7, 0, 3, 0], device=gpu)                      # any order, a row twice
    assert _same(m.scores(ratings, some, (60, 131), stage_cap=stage_cap), want[[7, 0, 3, 0], 60:131])
    uu, ii = torch.meshgrid(users, torch.arange(K.I, device=gpu), indexing="ij")
    pred = m.predict(ratings, uu.reshape(-1).contiguous(), ii.reshape(-1).contiguous())
    assert _same(pred.view(B, K.I), want)                              # predict(u, i) == scores[u, i] bit for bit
    clipped = m.predict(ratings, uu.reshape(-1).contiguous(), ii.reshape(-1).contiguous(), clip=(-1.0, 1.0))
    assert _same(clipped.view(B, K.I), np.clip(want, np.float32(-1.0), np.float32(1.0)))
    m.check()


def test_scores_of_the_fitted_users_with_a_full_table(gpu):
    m = _fit(gpu, K.base_case(), K.I, 200, 0.0, 1, weighted_average=False)
    users = torch.arange(K.U, device=gpu)
    got = m.scores(_dev(K.base_case(), gpu), users)
    assert _same(got, K.base_scores(200, 0.0, 1, False, 0.0, fitted=True))


def _seen_csr(exclude, gpu):
    rowptr = np.zeros(len(exclude) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(e) for e in exclude])
    col = np.array([c for e in exclude for c in e], np.int32)
    return torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)


@pytest.mark.parametrize("subset", [False, True])
def test_front_ends_rank_like_a_numpy_sort_of_the_reference_scores(gpu, subset):
    import deeprecommendation_amd as pkg
    m = _fit(gpu, K.base_case(), K.I, 7, 10.0, 2, fill=-3.5)
    ratings = _dev(K.score_case(), gpu)
    scores = K.base_scores(7, 10.0, 2, True, -3.5)
    B, k = scores.shape[0], 9
    rng = np.random.default_rng(11)
    item_ids = np.sort(rng.choice(K.I, 40, replace=False)) if subset else None
    C = 40 if subset else K.I
    exclude = [sorted(rng.choice(C, int(n), replace=False).tolist()) for n in rng.integers(0, 12, B)]
    exclude[0] = list(range(C - 4))                                    # fewer than k columns left
    targets = [sorted(rng.choice(C, 3, replace=False).tolist()) for _ in range(B)]
    ws, wp, wc, orders = K.ranked_ref(scores, k, item_ids, exclude)
    users = torch.arange(B, device=gpu)
    ids = None if item_ids is None else torch.from_numpy(item_ids).to(gpu)
    from deeprecommendation_amd import recommend
    for block_bytes in (recommend.BLOCK_BYTES, 4 * K.I * 3):       # one block of users; blocks of 3
        s, p, c = pkg.item_knn_top_k(m, ratings, users, k, item_ids=ids, exclude=_seen_csr(exclude, gpu), block_bytes=block_bytes)
        assert _same(s, ws) and np.array_equal(p.cpu().numpy(), wp) and np.array_equal(c.cpu().numpy(), wc)
        rank, ranked = pkg.item_knn_ranks(m, ratings, users, _seen_csr(targets, gpu), item_ids=ids, exclude=_seen_csr(exclude, gpu),
                                          block_bytes=block_bytes)
        want_rank = [int(np.flatnonzero(orders[b] == t)[0]) if t not in exclude[b] else -1 for b in range(B) for t in targets[b]]
        assert rank.cpu().tolist() == want_rank and ranked.cpu().tolist() == [len(o) for o in orders]
    assert wc[0] == 4 and (wc[1:] == k).all()
    met = pkg.ranking_metrics(rank, _seen_csr(targets, gpu)[0], ranked, cutoffs=(5,))     # the tuples are the ones the metrics take
    valid = [[r for r in want_rank[3 * b:3 * b + 3] if r >= 0] for b in range(B)]
    assert met["users"] == sum(1 for v in valid if v) and met["hr@5"] == pytest.approx(np.mean([min(v) < 5 for v in valid if v]))
    cov = pkg.catalogue_coverage(p, c, K.I)
    assert float(cov) == pytest.approx(len({int(x) for x in wp.reshape(-1) if x >= 0}) / K.I, rel=1e-12)   # a count over I, divided on the device


def test_bad_rows_raise_once_through_the_sticky_flags_and_nothing_is_read_through_them(gpu):
    from deeprecommendation_amd import native
    rowptr, col, val = (a.copy() for a in K.base_case())
    e = rowptr[K.LONG_USER + 1] - 1                                    # the last entry of the long row: far outside the items
    col[e] = 2 ** 31 - 1
    with pytest.raises(IndexError):
        _fit(gpu, (rowptr, col, val), K.I, 7, 0.0, 1, col_tile=64)
    native.check_oob(gpu), native.check_knn(gpu)               # raised once, then cleared
    col[e], col[rowptr[K.LONG_USER]] = K.base_case()[1][e], -7        # a negative column, first in its row: still ascending
    with pytest.raises(IndexError):
        _fit(gpu, (rowptr, col, val), K.I, 7, 0.0, 1)
    native.check_oob(gpu), native.check_knn(gpu)
    rowptr, col, val = (a.copy() for a in K.base_case())
    b = rowptr[20]
    col[b], col[b + 1] = col[b + 1], col[b]                            # user 20's first two columns swapped
    with pytest.raises(ValueError, match="ascending"):
        _fit(gpu, (rowptr, col, val), K.I, 7, 0.0, 1, col_tile=64)
    native.check_knn(gpu), native.check_oob(gpu)
    col[b + 1] = col[b]                                                # an item twice in a row
    with pytest.raises(ValueError, match="ascending"):
        _fit(gpu, (rowptr, col, val), K.I, 7, 0.0, 1)
    native.check_knn(gpu), native.check_oob(gpu)
    m = _fit(gpu, K.base_case(), K.I, 7, 0.0, 1)                       # a clean fit after all that: the reference table
    assert _table_same(m, K.base_table(7, 0.0, 1))
    ratings = _dev(K.score_case(), gpu)
    got = m.scores(ratings, torch.tensor([2, 8, -1, 4], device=gpu))   # rows 8 and -1 do not exist: they score as empty rows
    with pytest.raises(IndexError):
        m.check()
    m.check()
    want = K.base_scores(7, 0.0, 1, True, 0.0)
    assert _same(got[[0, 3]], want[[2, 4]]) and not got[[1, 2]].cpu().numpy().any()
    pred = m.predict(ratings, torch.tensor([2, 2, 9, 4], device=gpu), torch.tensor([10, K.I, 10, -1], device=gpu))
    with pytest.raises(IndexError):
        m.check()
    m.check()
    assert _same(pred[:1], want[2, 10:11]) and not pred[1:].cpu().numpy().any()
