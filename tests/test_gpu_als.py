"""GPU tests of the ImplicitALS baseline, bit for bit against the fp32 restatement of tests/als_ref.py: the chunked Gram matrix on every
row count, one half-sweep for every F on the base case and on the long case (rows of 0, 1, 64, 65, 512 and 1050 entries; the smallest
scratch buffer that holds one row's segments and the default), listed rows only, empty rows, each flag bit on the input the kernel
must refuse by checking, whole fits, the float64 loss, as_mf() under the project's ranking functions, fold-in, planted blocks, and
tools/implicit_baseline.py over three small sample files."""
import numpy as np
import pytest
import torch

import als_ref as A

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _dev(arrays, gpu):
    return tuple(torch.from_numpy(np.array(a)).to(gpu) for a in arrays)                 # a copy: the cached cases are read-only


def _clean(gpu):
    from deeprecommendation_amd import native
    native.check_als(gpu)


@pytest.mark.parametrize("F", [3, 64, 128])
@pytest.mark.parametrize("rows", A.GRAM_ROWS_LIST)
def test_gram_matches_the_chunked_sums_bit_for_bit(gpu, rows, F):
    from deeprecommendation_amd import native
    T, want = A.gram_case(rows, F)
    (t,) = _dev((T,), gpu)
    got = native.als_gram(t, F)                                        # ld = F + 5: the sentinel of the padding is never read
    assert _same(got, want) and torch.equal(got, got.t())
    assert np.abs(want).max() < 0.5 * rows + 1                         # no SENTINEL (7.25^2 per row) found its way in


def test_gram_of_no_rows_is_zero(gpu):
    from deeprecommendation_amd import native
    got = native.als_gram(torch.empty((0, 5), device=gpu), 5, out=torch.full((5, 5), 3.0, device=gpu))
    assert not got.any()


@pytest.mark.parametrize("F", A.F_LIST)
def test_half_sweep_matches_the_restatement_bit_for_bit(gpu, F):
    from deeprecommendation_amd import native
    rowptr, col, val = _dev(A.base_case(), gpu)
    (T,) = _dev((A.table(A.I, F, 100 + F),), gpu)
    G = native.als_gram(T)
    assert _same(G, A.base_gram(F))
    want, flag = A.base_sweep(F)
    assert flag == 0 and np.abs(want).max() > 0.1
    got = native.als_solve_rows(rowptr, col, val, torch.arange(A.U, device=gpu), T, G, A.ALPHA, A.REG)
    assert _same(got, want)
    assert not got[A.U - 1].any()                                      # the user without entries: zeros
    _clean(gpu)


@pytest.mark.parametrize("F", [3, 64, 128])
def test_long_rows_match_in_the_smallest_scratch_buffer_and_in_the_default(gpu, F):
    from deeprecommendation_amd import native
    rowptr, col, val = _dev(A.long_case(), gpu)
    (T,) = _dev((A.table(A.LONG_I, F, 300 + F, ld=F + 3, sd=0.1),), gpu)
    G = native.als_gram(T, F)
    want, flag = A.long_sweep(F)
    assert flag == 0
    rows = torch.arange(len(A.LONG_LENS), device=gpu)
    small = native.als_solve_rows(rowptr, col, val, rows, T, G, A.ALPHA, A.REG, block_bytes=3 * F * F * 4)     # the row's three segments
    assert _same(small, want)
    assert _same(native.als_solve_rows(rowptr, col, val, rows, T, G, A.ALPHA, A.REG), want)
    both = torch.tensor([0, 5, 0, 3], device=gpu)                      # the long row twice: two batches of the small buffer
    plan = native.als_plan(rowptr, both, F, 3 * F * F * 4)
    assert [(p[0], p[1], p[4]) for p in plan] == [(0, 2, 3), (2, 4, 3)]
    assert _same(native.als_solve_rows(rowptr, col, val, both, T, G, A.ALPHA, A.REG, plan=plan), want[[0, 5, 0, 3]])
    with pytest.raises(ValueError, match="block_bytes"):
        native.als_plan(rowptr, rows, F, 3 * F * F * 4 - 1)
    assert not want[1].any() and want[0].any() and want[2].any()
    _clean(gpu)


def test_listed_rows_only_are_written(gpu):
    from deeprecommendation_amd import native
    F = 33
    rowptr, col, val = _dev(A.base_case(), gpu)
    (T,) = _dev((A.table(A.I, F, 100 + F),), gpu)
    G = native.als_gram(T)
    want = A.base_sweep(F)[0]
    listed = [5, 0, 36, 17]
    out = torch.full((A.U, F + 2), A.SENTINEL, device=gpu)
    native.als_solve_rows(rowptr, col, val, torch.tensor(listed, device=gpu), T, G, A.ALPHA, A.REG, out=out, out_by_row=True)
    ref = np.full((A.U, F + 2), A.SENTINEL, np.float32)
    ref[listed, :F] = want[listed]
    assert _same(out, ref)
    got = native.als_solve_rows(rowptr, col, val, torch.tensor(listed, device=gpu), T, G, A.ALPHA, A.REG)
    assert _same(got, want[listed])
    _clean(gpu)


def _flag_case(gpu, F, rowptr, col, val, rows, T, G=None, **kw):
    from deeprecommendation_amd import native
    G = A.gram_ref(T, F) if G is None else G
    want, bits = A.solve_rows_ref(rowptr, col, val, rows, T, G, A.ALPHA, A.REG, F, **kw)
    d = _dev((rowptr, col, val, np.asarray(rows, np.int64), T, G), gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = None
    if kw.get("out_by_row"):
        out = torch.zeros((len(rowptr) - 1, F), device=gpu)
    got = native.als_solve_rows(*d, A.ALPHA, A.REG, out=out, out_by_row=bool(kw.get("out_by_row")), flag=flag)
    return got, want, int(flag.item()), bits


def test_each_flag_bit_is_set_by_its_own_fault(gpu):
    from deeprecommendation_amd import native
    F = 33
    rowptr, col, val = (a.copy() for a in A.base_case())
    T = A.table(A.I, F, 100 + F)
    clean = A.base_sweep(F)[0]
    rows = np.arange(A.U)
    r = int(np.argmax(np.diff(rowptr)))                                # the longest row: the faults below sit inside it
    assert rowptr[r + 1] - rowptr[r] >= 4
    # a column outside T: the entry is skipped, the rest of the row counts
    for at, bad in ((rowptr[r + 1] - 1, A.I + 3), (rowptr[r], -7)):
        c = col.copy()
        c[at] = bad
        got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, c, val, rows, T)
        assert bits == ref_bits == A.FLAG_COL and _same(got, want) and want[r].any() and not np.array_equal(want[r], clean[r])
        assert np.array_equal(np.delete(want, r, 0), np.delete(clean, r, 0))
    # a broken pointer pair and a listed row outside the CSR: zeros
    p = rowptr.copy()
    p[8] = -2                                                          # row 7 ends before it begins, row 8 begins outside the entries
    got, want, bits, ref_bits = _flag_case(gpu, F, p, col, val, rows, T)
    assert bits == ref_bits == A.FLAG_PTR and _same(got, want) and not want[7].any() and not want[8].any() and clean[7].any()
    assert np.array_equal(np.delete(want, [7, 8], 0), np.delete(clean, [7, 8], 0))
    p = rowptr.copy()
    p[-1] = len(col) + 5
    got, want, bits, ref_bits = _flag_case(gpu, F, p, col, val, rows, T)
    assert bits == ref_bits == A.FLAG_PTR and _same(got, want) and np.array_equal(want[:-1], clean[:-1])
    got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, col, val, np.array([3, A.U, -1, 2]), T)
    assert bits == ref_bits == A.FLAG_PTR and _same(got, want) and np.array_equal(want, np.stack([clean[3], np.zeros_like(clean[0]), np.zeros_like(clean[0]), clean[2]]))
    got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, col, val, np.array([3, A.U, -1, 2]), T, out_by_row=True)
    assert bits == ref_bits == A.FLAG_PTR and _same(got, want) and want[3].any() and not want[4].any()
    # a row whose columns do not strictly ascend: zeros
    c = col.copy()
    c[rowptr[r] + 1] = c[rowptr[r]]                                    # a pair given twice
    got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, c, val, rows, T)
    assert bits == ref_bits == A.FLAG_ORDER and _same(got, want) and not want[r].any()
    assert np.array_equal(np.delete(want, r, 0), np.delete(clean, r, 0))
    # a value that is negative or not finite: the entry is skipped
    for bad in (-0.5, np.inf, np.nan):
        v = val.copy()
        v[rowptr[r] + 2] = bad
        got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, col, v, rows, T)
        assert bits == ref_bits == A.FLAG_VAL and _same(got, want) and np.isfinite(want).all() and not np.array_equal(want[r], clean[r])
    # a pivot that is not positive: zeros for every row that is solved, none for the empty one
    G = A.gram_ref(T, F).copy()
    G[F - 2, F - 2] = -1e4
    got, want, bits, ref_bits = _flag_case(gpu, F, rowptr, col, val, rows, T, G=G)
    assert bits == ref_bits == A.FLAG_PIVOT and _same(got, want) and not want.any()
    f = native.als_flag(gpu)
    f.fill_(A.FLAG_ORDER | A.FLAG_VAL)
    with pytest.raises(ValueError, match="strictly ascend.*negative or not finite"):
        native.check_als(gpu)
    f.fill_(A.FLAG_COL | A.FLAG_PIVOT)
    with pytest.raises(IndexError, match="column outside.*pivot"):
        native.check_als(gpu)
    native.check_als(gpu)                                              # raised once, then cleared


def _base_samples(gpu, seed=3):
    rowptr, col, val = A.base_case()
    us = np.repeat(np.arange(A.U), np.diff(rowptr))
    perm = np.random.default_rng(seed).permutation(len(us))
    return _dev((us[perm], col.astype(np.int64)[perm], val[perm]), gpu)


@pytest.fixture(scope="module")
def fitted(gpu):
    import deeprecommendation_amd as pkg
    u, i, r = _base_samples(gpu)
    m = pkg.ImplicitALS(n_factors=A.FIT_F, n_iters=A.FIT_ITERS, reg=A.REG, alpha=A.ALPHA, init_sd=A.FIT_SD)
    return m.fit(u, i, r, A.U, A.I, generator=torch.Generator().manual_seed(A.FIT_SEED), track_loss=True)


def test_a_three_iteration_fit_equals_the_reference_fit_bit_for_bit(gpu, fitted):
    import deeprecommendation_amd as pkg
    X, Y, _ = A.base_fit()
    assert _same(fitted.user_factors_, X) and _same(fitted.item_factors_, Y)
    assert _same(fitted.item_gram_, A.gram_ref(Y, A.FIT_F))
    assert not X[A.U - 1].any() and not Y[A.I - 1].any() and np.abs(X).max() > 0.1
    rowptr, col, val = _dev(A.base_case(), gpu)
    again = pkg.ImplicitALS(n_factors=A.FIT_F, n_iters=A.FIT_ITERS, reg=A.REG, alpha=A.ALPHA, init_sd=A.FIT_SD)
    again.fit_csr(rowptr, col, val, A.I, generator=torch.Generator().manual_seed(A.FIT_SEED))
    assert _same(again.user_factors_, X) and _same(again.item_factors_, Y) and again.loss_ == []


def test_a_pair_given_twice_raises_from_check(gpu):
    import deeprecommendation_amd as pkg
    u, i, r = _base_samples(gpu)
    m = pkg.ImplicitALS(n_factors=3, n_iters=1, reg=A.REG, alpha=A.ALPHA)
    with pytest.raises(ValueError, match="strictly ascend"):
        m.fit(torch.cat([u, u[:1]]), torch.cat([i, i[:1]]), torch.cat([r, r[:1]]), A.U, A.I)
    m.check()                                                          # raised once, then cleared


def test_loss_matches_the_float64_objective_and_does_not_rise(gpu, fitted):
    rowptr, col, val = A.base_case()
    assert len(fitted.loss_) == 2 * A.FIT_ITERS
    want = A.base_fit()[2]                                             # the float64 objective of the (bit-equal) reference tables
    for got, w in zip(fitted.loss_, want):
        assert abs(got - w) <= 1e-9 * abs(w)
    last = A.objective64(rowptr, col, val, fitted.user_factors_.cpu().numpy(), fitted.item_factors_.cpu().numpy(), A.ALPHA, A.REG)
    assert abs(fitted.loss_[-1] - last) <= 1e-9 * abs(last)
    assert all(b <= a for a, b in zip(fitted.loss_, fitted.loss_[1:]))


def test_as_mf_tables_and_predictions(gpu, fitted):
    mf = fitted.as_mf()
    assert mf is fitted.as_mf() and not mf.training and mf.num_users == A.U and mf.num_items == A.I
    ue, ie = mf.user_embeddings[0], mf.item_embeddings[0]
    assert torch.equal(ue.weight.t(), fitted.user_factors_) and torch.equal(ie.weight.t(), fitted.item_factors_)
    assert not ue.bias.any() and not ie.bias.any() and not any(p.requires_grad for p in mf.parameters())
    g = torch.Generator().manual_seed(1)
    u, i = torch.randint(0, A.U, (200,), generator=g).to(gpu), torch.randint(0, A.I, (200,), generator=g).to(gpu)
    got = fitted.predict(u, i)
    prod = fitted.user_factors_.double()[u] * fitted.item_factors_.double()[i]
    assert (got.double() - prod.sum(1)).abs().max().item() <= A.FIT_F * 2.0 ** -23 * prod.abs().sum(1).max().item()
    assert not fitted.predict(torch.tensor([A.U - 1], device=gpu), torch.tensor([0], device=gpu)).any()


def test_as_mf_under_the_ranking_functions(gpu, fitted):
    import deeprecommendation_amd as pkg
    mf = fitted.as_mf()
    users = torch.arange(A.U, device=gpu)
    rowptr, col, val = _dev(A.base_case(), gpu)

    class R:
        pass
    ratings = R()
    ratings.rowptr, ratings.col = rowptr, col
    seen = pkg.rated_exclusion(ratings, users)
    a = pkg.top_k_items(mf, users, 5, exclude=seen, fused=True)
    b = pkg.top_k_items(mf, users, 5, exclude=seen, fused=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and (a[2] == 5).all()
    scores = fitted.predict(users.repeat_interleave(A.I), torch.arange(A.I, device=gpu).repeat(A.U)).view(A.U, A.I)
    assert torch.equal(a[0], scores.gather(1, a[1]))
    rated = torch.zeros((A.U, A.I), dtype=torch.bool, device=gpu)
    rated[torch.repeat_interleave(users, rowptr[1:] - rowptr[:-1]), col.long()] = True
    assert not rated.gather(1, a[1]).any()                             # nothing a user holds is recommended
    masked = torch.where(rated, torch.full_like(scores, float("-inf")), scores)
    assert torch.equal(a[0][:, 0], masked.max(1).values)
    tcol = a[1][:, 0].to(torch.int32)                                  # each user's best unrated item as the held-out one
    targets = (torch.arange(A.U + 1, device=gpu), tcol)
    rank, ranked = pkg.rank_of_items(mf, users, targets, exclude=seen)
    assert not rank.any() and torch.equal(ranked.long(), A.I - (rowptr[1:] - rowptr[:-1]))
    metrics = pkg.eval_full_ranking(mf, users, targets, exclude=seen, cutoffs=(1, 10))
    assert metrics["hr@1"] == 1.0 and metrics["ndcg@10"] == 1.0 and metrics["mrr"] == 1.0 and metrics["users"] == A.U


def test_fold_in_on_the_fitted_ratings_equals_the_user_half_sweep(gpu, fitted):
    rowptr, col, val = A.base_case()
    Y = fitted.item_factors_.cpu().numpy()
    want, flag = A.solve_rows_ref(rowptr, col, val, np.arange(A.U), Y, A.gram_ref(Y, A.FIT_F), A.ALPHA, A.REG, A.FIT_F)
    d = _dev((rowptr, col, val), gpu)
    got = fitted.fold_in_users(d, torch.arange(A.U, device=gpu))
    assert flag == 0 and _same(got, want)
    part = fitted.fold_in_users(d, torch.tensor([7, 36, 7, 0], device=gpu))
    assert _same(part, want[[7, 36, 7, 0]]) and not part[1].any()
    fitted.check()


def test_recommend_new_users_is_top_k_on_the_folded_vectors(gpu, fitted):
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.baselines import _mf_of_tables
    new = (np.array([0, 3, 3, 8], np.int64), np.array([1, 4, 9, 0, 2, 5, 11, 20], np.int32),
           np.array([1, 0.5, 3, 2, 2, 5, 4.5, 1], np.float32))       # three new users over the fitted items, one without entries
    d = _dev(new, gpu)
    rows = torch.arange(3, device=gpu)
    vec = fitted.fold_in_users(d, rows)
    mf = _mf_of_tables(vec, fitted.item_factors_)

    class R:
        pass
    ratings = R()
    ratings.rowptr, ratings.col = d[0], d[1]
    for exclude_rated in (True, False):
        got = fitted.recommend_new_users(d, rows, 4, exclude_rated=exclude_rated)
        want = pkg.top_k_items(mf, rows, 4, exclude=pkg.rated_exclusion(ratings, rows) if exclude_rated else None)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    held = fitted.recommend_new_users(d, rows, 4)[1]
    assert not np.isin(held[0].cpu().numpy(), [1, 4, 9]).any() and not np.isin(held[2].cpu().numpy(), [0, 2, 5, 11, 20]).any()
    fitted.check()


def test_fit_dataset_is_the_fit_on_the_providers_positions(gpu):
    """12 users x 9 items with raw ids (users 3 p + 30, items 7 p + 7), 40 distinct pairs in shuffled order: the tables of fit_dataset
    are fit's on the provider's positions, bit for bit."""
    import pandas as pd
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset
    U, I = 12, 9
    rng = np.random.RandomState(5)
    pairs = rng.permutation(U * I)[:40]
    frame = pd.DataFrame({"userId": pairs // I * 3 + 30, "movieId": pairs % I * 7 + 7, "rating": rng.randint(1, 11, 40) * 0.5})
    cp = IndexProvider(np.arange(U) * 3 + 30, np.arange(I) * 7 + 7)
    kw = dict(n_factors=4, n_iters=2, reg=A.REG, alpha=A.ALPHA)
    a = pkg.ImplicitALS(**kw).fit_dataset(FixedPointwiseDataset(frame, cp), gpu, generator=torch.Generator().manual_seed(1))
    u = torch.from_numpy(np.asarray(cp.get_user_profile(frame["userId"].values), dtype=np.int64)).to(gpu)
    i = torch.from_numpy(np.asarray(cp.get_item_profile(frame["movieId"].values), dtype=np.int64)).to(gpu)
    r = torch.from_numpy(frame["rating"].to_numpy(dtype=np.float32)).to(gpu)
    b = pkg.ImplicitALS(**kw).fit(u, i, r, U, I, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a.user_factors_, b.user_factors_) and torch.equal(a.item_factors_, b.item_factors_) and torch.equal(a.item_gram_, b.item_gram_)
    assert a.user_factors_.shape == (U, 4) and a.item_factors_.shape == (I, 4) and a.user_factors_.any() and a.item_factors_.any()
    assert torch.equal(u, torch.from_numpy(pairs // I).to(gpu)) and torch.equal(i, torch.from_numpy(pairs % I).to(gpu))


def test_planted_blocks_come_back_with_hit_rate_one(gpu):
    import deeprecommendation_amd as pkg
    (rowptr, col, val), held = A.planted_case()
    n = A.PLANT_G * A.PLANT_N
    X, Y = A.planted_fit()
    S = X.astype(np.float64) @ Y.astype(np.float64).T
    S[np.repeat(np.arange(n), np.diff(rowptr)), col] = -np.inf
    assert (S.argmax(1) == held).all()                                 # the reference fit on the CPU: HR@1 = 1.0
    d = _dev((rowptr, col, val), gpu)
    m = pkg.ImplicitALS(n_factors=A.PLANT_F, n_iters=A.PLANT_ITERS, reg=A.REG, alpha=A.ALPHA, init_sd=A.FIT_SD)
    m.fit_csr(*d, n, generator=torch.Generator().manual_seed(A.FIT_SEED))
    assert _same(m.user_factors_, X) and _same(m.item_factors_, Y)
    users = torch.arange(n, device=gpu)
    targets = (torch.arange(n + 1, device=gpu), torch.from_numpy(held.astype(np.int32)).to(gpu))

    class R:
        pass
    ratings = R()
    ratings.rowptr, ratings.col = d[0], d[1]
    metrics = pkg.eval_full_ranking(m.as_mf(), users, targets, exclude=pkg.rated_exclusion(ratings, users), cutoffs=(1,))
    assert metrics["hr@1"] == 1.0 and metrics["users"] == n


def test_implicit_baseline_tool_searches_the_grid_and_scores_the_best(gpu, tmp_path, monkeypatch, capsys):
    import importlib.util
    import os
    import pandas as pd
    from conftest import ROOT
    (rowptr, col, val), held = A.planted_case()
    n = A.PLANT_G * A.PLANT_N
    us = np.repeat(np.arange(n), np.diff(rowptr))
    last = rowptr[1:] - 1                                              # each user's last planted item goes to VAL, the held-out one to TEST
    keep = np.ones(len(col), bool)
    keep[last] = False

    def frame(u, i):
        return pd.DataFrame({"userId": u * 3 + 5, "movieId": i.astype(np.int64) * 7 + 2, "rating": np.full(len(u), 4.0)})

    for name, f in (("train", frame(us[keep], col[keep])), ("val", frame(us[last], col[last])), ("test", frame(np.arange(n), held))):
        f.to_csv(tmp_path / (name + ".csv"), index=False)
    spec = importlib.util.spec_from_file_location("implicit_baseline_tool", os.path.join(ROOT, "tools", "implicit_baseline.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr("sys.argv", ["implicit_baseline.py", str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "test.csv"), "--factors", "4", "8",
                                     "--regs", "0.1", "--alphas", "1", "4", "--iters", "6"])
    tool.main()
    lines = capsys.readouterr().out.strip().splitlines()
    grid = [l for l in lines if l.startswith("factors=")]
    assert [l.split(":")[0] for l in grid] == [f"factors={f} reg=0.1 alpha={a} iters=6" for f in (4, 8) for a in (1.0, 4.0)]
    ndcg = [float(l.split("NDCG@10 ")[1].split(",")[0]) for l in grid]
    assert all(f"({n} users)" in l for l in grid) and all(0.0 < v <= 1.0 for v in ndcg)
    best = lines[len(grid)]
    assert best.startswith("best by val NDCG@10:") and grid[int(np.argmax(ndcg))].split(":")[0].replace(" iters=6", "") in best
    assert f"(val NDCG@10 {max(ndcg):.4f})" in best
    assert lines[-1].startswith("test HR@10 ") and f"({n} users)" in lines[-1] and 0.0 < float(lines[-1].split()[2].rstrip(",")) <= 1.0
