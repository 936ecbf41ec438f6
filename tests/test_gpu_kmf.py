"""GPU tests of the KernelMF baseline: ncf_kmf_epoch and ncf_kmf_fold_users against the fp32 loops of tests/kmf_ref.py bit for bit
(tables, biases, the float64 loss partials, untouched padding, repeatability, 3 epochs = 3 x 1), the three flags on inputs the kernel
must refuse by checking, KernelMF.fit / fit_dataset / update_users against the same reference, as_mf() under the project's ranking
functions, and tools/cf_baseline.py over three small sample files."""
import math

import numpy as np
import pytest
import torch

import kmf_ref as K

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _dev_plan(plan, gpu):
    return {k: torch.from_numpy(np.ascontiguousarray(plan[k])).to(gpu) for k in ("user", "item", "rating", "block_ptr", "user_block", "item_block")}


def _tables(P0, Q0, F, pad, gpu):
    ld = K.leading_dim(F, pad)
    return torch.from_numpy(K.padded(P0, F, ld)).to(gpu), torch.from_numpy(K.padded(Q0, F, ld)).to(gpu)


def _run(gpu, F, plan, mu, pad, calls, start=None):
    """``calls``: the n_epochs of successive ncf_kmf_epoch calls from the start tables.  Returns (PU, QI, sse, flag) on the host."""
    from deeprecommendation_amd import native
    P0, Q0 = start if start is not None else K.init_tables(F)
    PU, QI = _tables(P0, Q0, F, pad, gpu)
    d = _dev_plan(plan, gpu)
    sse = torch.zeros((sum(calls), plan["W"]), dtype=torch.float64, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    done = 0
    for e in calls:
        native.kmf_epoch(PU, QI, F, d["user"], d["item"], d["rating"], d["block_ptr"], d["user_block"], d["item_block"], float(mu), K.LR,
                         K.REG, e, sse=sse[done:done + e], flag=flag)
        done += e
    torch.cuda.synchronize()
    return PU.cpu().numpy(), QI.cpu().numpy(), sse.cpu().numpy(), int(flag.item())


def _check(got, want, F, what):
    PU, QI, sse, flag = got
    P, Q, ref_sse = want
    assert flag == 0, what
    assert _same(PU[:, :F + 1], P) and _same(QI[:, :F + 1], Q), what
    assert _same(sse, ref_sse), what
    assert (PU[:, F + 1:] == K.SENTINEL).all() and (QI[:, F + 1:] == K.SENTINEL).all(), what


@pytest.mark.parametrize("W", K.W_LIST)
@pytest.mark.parametrize("F", K.F_LIST)
def test_epoch_equals_the_fp32_loop_bit_for_bit(gpu, F, W):
    mu, plan = K.ratings_case()[3], K.plan_case(W)
    one, three = K.epoch_case(F, W)
    for pad in (True, False):
        _check(_run(gpu, F, plan, mu, pad, [1]), one, F, (pad, 1))
        first = _run(gpu, F, plan, mu, pad, [3])
        _check(first, three, F, (pad, 3))
        again = _run(gpu, F, plan, mu, pad, [3])
        assert all(_same(a, b) for a, b in zip(first[:3], again[:3])), pad
        _check(_run(gpu, F, plan, mu, pad, [1, 1, 1]), three, F, (pad, "3 x 1"))


@pytest.mark.parametrize("F,W", [(1, 1), (65, 1), (65, 5), (256, 5)])
def test_a_single_sample(gpu, F, W):
    mu, plan = K.ratings_case(1)[3], K.plan_case(W, 1)
    one, three = K.epoch_case(F, W, n=1)
    for pad in (True, False):
        _check(_run(gpu, F, plan, mu, pad, [1]), one, F, pad)
        _check(_run(gpu, F, plan, mu, pad, [3]), three, F, pad)


def _without(plan, k):
    """The plan with stored sample k taken out."""
    out = dict(plan)
    for key in ("user", "item", "rating"):
        out[key] = np.delete(plan[key], k)
    ptr = plan["block_ptr"].copy()
    ptr[ptr > k] -= 1
    out["block_ptr"] = ptr
    return out


def _flag_case(gpu, F, W, broken, remaining, bit):
    mu = K.ratings_case()[3]
    P, Q = K.init_tables(F)
    want_sse = K.epoch_ref(P, Q, F, remaining, mu, K.LR, K.REG, 2)
    Pc, Qc = K.init_tables(F)
    chk_sse, chk_flag = K.epoch_ref_flags(Pc, Qc, F, broken, mu, K.LR, K.REG, 2)     # the restated checks skip the same samples
    assert chk_flag == bit and _same(Pc, P) and _same(Qc, Q) and _same(chk_sse, want_sse)
    for pad in (True, False):
        PU, QI, sse, flag = _run(gpu, F, broken, mu, pad, [2])
        assert flag == bit, pad
        assert _same(PU[:, :F + 1], P) and _same(QI[:, :F + 1], Q) and _same(sse, want_sse), pad
        assert (PU[:, F + 1:] == K.SENTINEL).all() and (QI[:, F + 1:] == K.SENTINEL).all(), pad


@pytest.mark.parametrize("which", ["item past the table", "negative user"])
def test_an_id_out_of_range_sets_bit_0_and_is_skipped(gpu, which):
    F, W = 65, 5
    plan = K.plan_case(W)
    k = int(plan["block_ptr"][7]) + 1                     # the second sample of block 7
    assert k < plan["block_ptr"][8]
    broken = dict(plan)
    if which == "item past the table":
        broken["item"] = plan["item"].copy()
        broken["item"][k] = K.I
    else:
        broken["user"] = plan["user"].copy()
        broken["user"][k] = -1
    _flag_case(gpu, F, W, broken, _without(plan, k), 1)


def test_a_sample_filed_in_the_wrong_block_sets_bit_1_and_is_skipped(gpu):
    F, W = 65, 5
    plan = K.plan_case(W)
    k = int(plan["block_ptr"][7]) + 1
    a = plan["user_block"][plan["user"][k]]
    other = int(np.flatnonzero(plan["user_block"] != a)[0])             # a user of another block, in this block's slot
    broken = dict(plan)
    broken["user"] = plan["user"].copy()
    broken["user"][k] = other
    _flag_case(gpu, F, W, broken, _without(plan, k), 2)


def test_a_decreasing_block_ptr_pair_sets_bit_2_and_empties_the_block(gpu):
    F, W = 65, 5
    plan = K.plan_case(W)
    ptr = plan["block_ptr"]
    assert ptr[-1] - ptr[-2] >= 2                         # the last block holds samples; only its own pair is broken
    broken = dict(plan)
    broken["block_ptr"] = ptr.copy()
    broken["block_ptr"][-1] = ptr[-2] - 1
    remaining = dict(plan)
    remaining["block_ptr"] = ptr.copy()
    remaining["block_ptr"][-1] = ptr[-2]                  # the same plan with the last block empty (its samples are never reached)
    _flag_case(gpu, F, W, broken, remaining, 4)


@pytest.mark.parametrize("F", [3, 65, 256])
def test_fold_users_equals_the_fp32_loop_bit_for_bit(gpu, F):
    from deeprecommendation_amd import native
    users, rowptr, col, rating = K.fold_case(F)
    mu = 2.75
    P0, Q0 = K.init_tables(F)
    P0[K.U - 1] = 0.0                                     # a user without training ratings starts from zero
    P, Q = P0.copy(), Q0.copy()
    want_sse, want_flag = K.fold_users_ref(P, Q, F, users, rowptr, col, rating, mu, K.LR, K.REG, 3)
    assert want_flag == 0 and _same(Q, Q0)
    others = np.setdiff1d(np.arange(K.U), users)
    for pad in (True, False):
        PU, QI = _tables(P0, Q0, F, pad, gpu)
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        sse = native.kmf_fold_users(PU, QI, F, *(torch.from_numpy(a).to(gpu) for a in (users, rowptr, col, rating)), mu, K.LR, K.REG, 3, flag=flag)
        PU, QI = PU.cpu().numpy(), QI.cpu().numpy()
        assert int(flag.item()) == 0
        assert _same(PU[:, :F + 1], P) and _same(sse.cpu().numpy(), want_sse), pad
        assert _same(QI, K.padded(Q0, F, QI.shape[1])) and _same(PU[others], K.padded(P0, F, PU.shape[1])[others]), pad
        assert (PU[:, F + 1:] == K.SENTINEL).all(), pad


def test_fold_users_flags_what_it_skips(gpu):
    from deeprecommendation_amd import native
    F = 65
    users, rowptr, col, rating = K.fold_case(F)
    users, col, rowptr = users.copy(), col.copy(), rowptr.copy()
    users[3] = K.U                                        # a user outside the table: its row of the CSR is skipped
    col[2] = -1                                           # one item of user 3 outside the table: that sample is skipped
    P0, Q0 = K.init_tables(F)
    P, Q = P0.copy(), Q0.copy()
    want_sse, want_flag = K.fold_users_ref(P, Q, F, users, rowptr, col, rating, 2.75, K.LR, K.REG, 2)
    assert want_flag == 1
    PU, QI = _tables(P0, Q0, F, True, gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    sse = native.kmf_fold_users(PU, QI, F, *(torch.from_numpy(a).to(gpu) for a in (users, rowptr, col, rating)), 2.75, K.LR, K.REG, 2, flag=flag)
    assert int(flag.item()) == 1 and _same(PU.cpu().numpy()[:, :F + 1], P) and _same(sse.cpu().numpy(), want_sse)
    bad = rowptr.copy()
    bad[1] = rowptr[2] + 1                                # rows 0 and 1 now end / start past each other: row 1 decreases
    P, Q = P0.copy(), Q0.copy()
    want_sse, want_flag = K.fold_users_ref(P, Q, F, users, bad, col, rating, 2.75, K.LR, K.REG, 1)
    assert want_flag & 4
    PU, QI = _tables(P0, Q0, F, True, gpu)
    flag.zero_()
    sse = native.kmf_fold_users(PU, QI, F, *(torch.from_numpy(a).to(gpu) for a in (users, bad, col, rating)), 2.75, K.LR, K.REG, 1, flag=flag)
    assert int(flag.item()) == want_flag and _same(PU.cpu().numpy()[:, :F + 1], P) and _same(sse.cpu().numpy(), want_sse)


# ---------------------------------------------------------------------------------------------- KernelMF
FIT_F, FIT_W, FIT_SEED = 65, 5, 7


def _samples(gpu):
    us, it, r, mu = K.ratings_case()
    return torch.from_numpy(us.copy()).to(gpu), torch.from_numpy(it.copy()).to(gpu), torch.from_numpy(r.copy()).to(gpu), mu


def _fit(gpu, n_epochs, **kw):
    import deeprecommendation_amd as pkg
    u, i, r, _ = _samples(gpu)
    m = pkg.KernelMF(n_factors=FIT_F, n_epochs=n_epochs, lr=K.LR, reg=K.REG, n_blocks=FIT_W)
    return m.fit(u, i, r, K.U, K.I, generator=torch.Generator().manual_seed(FIT_SEED), **kw)


@pytest.fixture(scope="module")
def fitted(gpu):
    return _fit(gpu, 3)


@pytest.fixture(scope="module")
def fit_reference():
    """The fit restated: the generator's two draws, zero biases, zero rows for ids without a rating, 3 epochs of epoch_ref."""
    g = torch.Generator().manual_seed(FIT_SEED)
    P = np.zeros((K.U, FIT_F + 1), np.float32)
    Q = np.zeros((K.I, FIT_F + 1), np.float32)
    P[:, :FIT_F] = torch.empty(K.U, FIT_F).normal_(0.0, 0.1, generator=g).numpy()
    Q[:, :FIT_F] = torch.empty(K.I, FIT_F).normal_(0.0, 0.1, generator=g).numpy()
    us, it, r, mu = K.ratings_case()
    P[np.bincount(us, minlength=K.U) == 0] = 0.0
    Q[np.bincount(it, minlength=K.I) == 0] = 0.0
    sse1 = K.epoch_ref(P, Q, FIT_F, K.plan_case(FIT_W), mu, K.LR, K.REG, 1)
    one = (P.copy(), Q.copy())
    sse = np.concatenate([sse1, K.epoch_ref(P, Q, FIT_F, K.plan_case(FIT_W), mu, K.LR, K.REG, 2)])
    rmse = []
    for row in sse:
        acc = 0.0
        for v in row:
            acc = acc + float(v)
        rmse.append(math.sqrt(acc / K.N))
    return one, (P, Q), rmse


def test_fit_equals_the_reference_fit(gpu, fitted, fit_reference):
    _, (P, Q), rmse = fit_reference
    F = FIT_F
    assert fitted.n_blocks_ == FIT_W and fitted.global_mean_ == float(K.ratings_case()[3])
    assert fitted.user_table_.shape[1] % 32 == 0 and fitted.user_table_.shape[1] >= F + 1
    pu, qi = fitted.user_table_.cpu().numpy(), fitted.item_table_.cpu().numpy()
    assert _same(pu[:, :F + 1], P) and _same(qi[:, :F + 1], Q)
    assert not pu[:, F + 1:].any() and not qi[:, F + 1:].any()
    assert fitted.train_rmse_ == rmse and rmse[0] > rmse[1] > rmse[2]
    assert not pu[K.U - 1].any() and not qi[K.I - 1].any() and pu[0].any()       # the ids without a rating
    fitted.check()


def test_at_epochs_calls_back_with_the_shorter_fit(gpu, fit_reference):
    (P1, Q1), _, rmse = fit_reference
    seen = []

    def cb(model, epoch):
        seen.append((epoch, model.user_table_.clone(), model.item_table_.clone(), list(model.train_rmse_)))

    _fit(gpu, 3, epoch_callback=cb, at_epochs=(1, 3))
    assert [s[0] for s in seen] == [1, 3]
    short = _fit(gpu, 1)
    assert torch.equal(seen[0][1], short.user_table_) and torch.equal(seen[0][2], short.item_table_)
    assert _same(seen[0][1].cpu().numpy()[:, :FIT_F + 1], P1) and _same(seen[0][2].cpu().numpy()[:, :FIT_F + 1], Q1)
    assert seen[0][3] == rmse[:1] == short.train_rmse_ and seen[1][3] == rmse


def test_as_mf_tables_and_predictions(gpu, fitted):
    F = FIT_F
    mf = fitted.as_mf()
    assert mf is fitted.as_mf() and not mf.training and mf.num_users == K.U and mf.num_items == K.I
    pu, qi = fitted.user_table_, fitted.item_table_
    mu = torch.tensor(fitted.global_mean_, dtype=torch.float32, device=gpu)
    ut = torch.cat([pu[:, :F], (pu[:, F] + mu)[:, None], torch.ones(K.U, 1, device=gpu)], 1)
    it = torch.cat([qi[:, :F], torch.ones(K.I, 1, device=gpu), qi[:, F:F + 1]], 1)
    ue, ie = mf.user_embeddings[0], mf.item_embeddings[0]
    assert torch.equal(ue.weight.t(), ut) and torch.equal(ie.weight.t(), it) and not ue.bias.any() and not ie.bias.any()
    u = torch.arange(K.U, device=gpu).repeat_interleave(K.I)
    i = torch.arange(K.I, device=gpu).repeat(K.U)
    with torch.no_grad():
        raw = mf(u, i).view(-1)
    assert torch.equal(fitted.predict(u, i, clip=False), raw)
    assert torch.equal(fitted.predict(u, i), raw.clamp(fitted.min_rating, fitted.max_rating))
    # what the table computes, in float64: mu + b_u + b_i + p.q within the fp32 error of F + 2 products of entries below 1 in sum
    want = (ut.double()[u] * it.double()[i]).sum(1)
    assert (raw.double() - want).abs().max().item() <= (F + 2) * 2.0 ** -23 * (ut.double()[u] * it.double()[i]).abs().sum(1).max().item()
    unseen = fitted.predict(torch.tensor([K.U - 1], device=gpu), torch.tensor([0], device=gpu), clip=False)
    assert unseen.item() == (mu + qi[0, F]).item()        # a user without ratings: mu plus the known side's bias, one rounding


def test_as_mf_under_the_ranking_functions(gpu, fitted, tmp_path):
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    from deeprecommendation_amd.neural_collaborative_filtering.util import load_model
    mf = fitted.as_mf()
    users = torch.arange(K.U, device=gpu)
    a = pkg.top_k_items(mf, users, 5, fused=True)
    b = pkg.top_k_items(mf, users, 5, fused=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and (a[2] == 5).all()
    scores = fitted.predict(users.repeat_interleave(K.I), torch.arange(K.I, device=gpu).repeat(K.U), clip=False).view(K.U, K.I)
    assert torch.equal(a[0], scores.gather(1, a[1]))
    rowptr = torch.arange(K.U + 1, device=gpu)
    col = (torch.arange(K.U, device=gpu) % K.I).to(torch.int32)
    rank, ranked = pkg.rank_of_items(mf, users, (rowptr, col))
    assert (ranked == K.I).all() and rank.shape == (K.U,) and ((rank >= 0) & (rank < K.I)).all()
    hit = rank < 5
    assert torch.equal(hit, (a[1] == col.long()[:, None]).any(1))
    path = str(tmp_path / "kmf.pt")
    mf.save_model(path)
    back = load_model(path, MF).to(gpu).eval()
    with torch.no_grad():
        assert torch.equal(back(users, col.long()), mf(users, col.long()))


def _frames():
    """The rank-4 case as three sample files' worth of rows with raw ids (users 3 p + 30, items 7 p + 7); the last 100 rows are held out."""
    import pandas as pd
    us, it, r, _ = K.ratings_case()
    frame = pd.DataFrame({"userId": us * 3 + 30, "movieId": it * 7 + 7, "rating": r.astype(np.float64)})
    return frame.iloc[:450], frame.iloc[450:500], frame.iloc[500:]


def test_fit_dataset_is_the_fit_on_the_providers_positions(gpu):
    import deeprecommendation_amd as pkg
    from deeprecommendation_amd.content_providers.index_providers import IndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset
    train = _frames()[0]
    cp = IndexProvider(np.arange(K.U) * 3 + 30, np.arange(K.I) * 7 + 7)
    kw = dict(n_factors=8, n_epochs=2, lr=K.LR, reg=K.REG, n_blocks=3)
    a = pkg.KernelMF(**kw).fit_dataset(FixedPointwiseDataset(train, cp), gpu, generator=torch.Generator().manual_seed(1))
    u = torch.from_numpy(np.asarray(cp.get_user_profile(train["userId"].values), dtype=np.int64)).to(gpu)
    i = torch.from_numpy(np.asarray(cp.get_item_profile(train["movieId"].values), dtype=np.int64)).to(gpu)
    r = torch.from_numpy(train["rating"].to_numpy(dtype=np.float32)).to(gpu)
    b = pkg.KernelMF(**kw).fit(u, i, r, K.U, K.I, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a.user_table_, b.user_table_) and torch.equal(a.item_table_, b.item_table_) and a.train_rmse_ == b.train_rmse_
    assert a.user_table_.shape[0] == K.U and a.item_table_.shape[0] == K.I and len(a.train_rmse_) == 2


def test_cf_baseline_tool_searches_the_grid_and_scores_the_best(gpu, tmp_path, monkeypatch, capsys):
    import importlib.util
    import os
    from conftest import ROOT
    for name, frame in zip(("train", "val", "test"), _frames()):
        frame.to_csv(tmp_path / (name + ".csv"), index=False)
    spec = importlib.util.spec_from_file_location("cf_baseline_tool", os.path.join(ROOT, "tools", "cf_baseline.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr("sys.argv", ["cf_baseline.py", str(tmp_path / "train"), str(tmp_path / "val"), str(tmp_path / "test.csv"), "--factors", "4", "8",
                                     "--lrs", "0.05", "--regs", "0.02", "--epochs", "2", "4", "--blocks", "3"])
    tool.main()
    lines = capsys.readouterr().out.strip().splitlines()
    grid = [l for l in lines if l.startswith("factors=")]
    assert [l.split(":")[0] for l in grid] == [f"factors={f} lr=0.05 reg=0.02 epochs={e}" for f in (4, 8) for e in (2, 4)]
    val = [float(l.split("val MSE ")[1].split(",")[0]) for l in grid]
    best = lines[len(grid)]
    assert best.startswith("best by val MSE:") and grid[int(np.argmin(val))].split(":")[0] in best and "blocks=3" in best
    assert lines[-2].startswith("test MSE ") and f"(val MSE {min(val):.4f})" in lines[-2]
    assert lines[-1].startswith("test NDCG@10 ") and 0.0 < float(lines[-1].split()[2].rstrip(",")) <= 1.0


def test_update_users_folds_in_against_the_fixed_item_table(gpu):
    m = _fit(gpu, 1)
    F = FIT_F
    users, rowptr, col, rating = K.fold_case(F)
    P, Q = m.user_table_.cpu().numpy()[:, :F + 1].copy(), m.item_table_.cpu().numpy()[:, :F + 1].copy()
    want_sse, _ = K.fold_users_ref(P, Q, F, users, rowptr, col, rating, np.float32(m.global_mean_), 0.03, K.REG, 2)
    before = m.item_table_.clone()
    mf = m.as_mf()
    dev = [torch.from_numpy(a).to(gpu) for a in (rowptr, col, rating)]
    sse = m.update_users(*dev, torch.from_numpy(users.astype(np.int64)).to(gpu), n_epochs=2, lr=0.03)
    assert _same(m.user_table_.cpu().numpy()[:, :F + 1], P) and _same(sse.cpu().numpy(), want_sse) and torch.equal(m.item_table_, before)
    assert m.user_table_[K.U - 1].any() and m.as_mf() is not mf              # the user without training ratings has a row now
    with pytest.raises(ValueError):
        m.update_users(*dev, torch.tensor([3, 3, 11, 0], device=gpu))
