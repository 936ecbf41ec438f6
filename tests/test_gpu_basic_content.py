"""GPU: the content form of BasicNCF as a table model.  ``set_content`` attaches the (U, F) profile and (I, F) feature tables; int64
forwards then name their rows and run through the table kernels.  Pinned against the reference fixture and against the float-row
forward (unchanged code) at tests/test_gpu_basic.py's bar; the training step against the float-row step bit for bit; the ranking
front end (top_k_items, rank_of_items, eval_model resident) against its unfused / loader routes; the profile builder through the
providers; and the content-based cosine baseline against a float64 restatement."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from content_cosine_ref import ITEMS as COS_ITEMS, K as COS_K, TOL as COS_TOL, USERS as COS_USERS, ZERO_USER, cosine_case, decided, undecided_share
from test_gpu_basic import assert_close
from user_profiles_ref import profiles_loop

pytestmark = pytest.mark.gpu

F, U, I = 67, 300, 500


def _second_shape(gpu, seed=11, dropout_rate=0.2):
    """emb 64 / 64, MLP [256, 128] over F = 67 content columns, 300 profiles and 500 items."""
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    torch.manual_seed(seed)
    m = BasicNCF(item_dim=F, user_dim=F, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128], dropout_rate=dropout_rate).eval().to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    prof, feat = (torch.randn(U, F, generator=g) * 0.3).to(gpu), torch.randn(I, F, generator=g).to(gpu)
    return m, prof, feat


def _pairs(gpu, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, U, (B,), generator=g).to(gpu), torch.randint(0, I, (B,), generator=g).to(gpu)


def _equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ----------------------------------------------------------------------------- model
def test_reference_fixture_through_the_indexed_route(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    state, a, kw = load_golden("g1_basic_dense_profiles")
    m = BasicNCF(**kw)
    m.load_state_dict(state)
    m = m.eval().to(gpu)
    xu, xi = torch.from_numpy(a["X_user"]).float().to(gpu), torch.from_numpy(a["X_item"]).float().to(gpu)
    assert m.set_content(xu, xi) is m and m.num_users == xu.shape[0] and m.num_items == xi.shape[0]
    idx = torch.arange(xu.shape[0], device=gpu)
    with torch.no_grad():
        out = m(idx, idx)
        rev = m(idx.flip(0), idx.flip(0))
    assert_close(out, torch.from_numpy(a["out"]))
    assert_close(rev, torch.from_numpy(a["out"]).flip(0))
    m.set_content(None, None)
    assert m.num_users == kw["user_dim"] and m.num_items == kw["item_dim"]


def test_indexed_forward_matches_the_float_row_forward(gpu):
    from deeprecommendation_amd import native
    m, prof, feat = _second_shape(gpu)
    u, i = _pairs(gpu, 1000)
    with torch.no_grad():
        rows = m(prof[u], feat[i])                       # unchanged code, pinned to the reference
        assert m.set_content(prof, feat).num_items == I and m.num_users == U
        again = m(prof[u], feat[i])                      # float rows with content attached: exactly as before
        out = m(u, i)
        m.set_partial_first_layer(True)
        part = m(u, i)
        m.set_partial_first_layer(None).set_fold_first_layer(True)
        fold = m(u, i)
        m.set_fold_first_layer(False)
    assert torch.equal(rows, again)
    assert_close(out, rows)
    assert torch.equal(part, out)                        # the partial-layer scorer owns the cached table: bit-identical by its contract
    assert_close(fold, rows)
    native.check_oob(gpu)
    with torch.no_grad():
        m(torch.tensor([U], device=gpu), torch.tensor([0], device=gpu))
    with pytest.raises(IndexError):                      # a position is a row of the content table, not a feature column
        native.check_oob(gpu)


def test_tables_follow_the_weights_and_the_content(gpu):
    m, prof, feat = _second_shape(gpu)
    u, i = _pairs(gpu, 200)
    m.set_content(prof, feat)
    with torch.no_grad():
        before = m(u, i)
        m.user_embeddings[0].weight.mul_(1.5)            # in place: the parameter's version moves, the cache key with it
        after = m(u, i)
        rows = m(prof[u], feat[i])
        m.set_content(prof * 2, feat)
        doubled = m(u, i)
        rows2 = m(prof[u] * 2, feat[i])
    assert not torch.equal(before, after)
    assert_close(after, rows)
    assert_close(doubled, rows2)


def _graph_ops(t):
    """The names of the autograd nodes behind ``t``, depth first."""
    names, stack, seen = [], [t.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def test_training_step_equals_the_float_row_step_bit_for_bit(gpu):
    m, prof, feat = _second_shape(gpu)
    m.train()
    u, i = _pairs(gpu, 513)
    y = torch.rand(513, 1, device=gpu) * 5

    def step(xu, xi):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(21)                            # the hidden layers' dropout draws from torch's stream
        loss = torch.nn.functional.mse_loss(m(xu, xi), y)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, _graph_ops(loss)

    loss_rows, grads_rows, ops_rows = step(prof[u], feat[i])
    m.set_content(prof, feat)
    loss_idx, grads_idx, ops_idx = step(u, i)
    assert torch.equal(loss_rows, loss_idx) and float(loss_rows) > 0
    assert grads_rows.keys() == grads_idx.keys() and all(g is not None for g in grads_idx.values())
    for k in grads_rows:
        assert torch.equal(grads_rows[k].view(torch.int32), grads_idx[k].view(torch.int32)), k
    assert ops_rows == ops_idx and any("LinearFn" in n for n in ops_idx)


# ----------------------------------------------------------------------------- ranking front end
@pytest.fixture
def mlp_calls(monkeypatch):
    from deeprecommendation_amd import native
    calls = {"mlp_topk": 0, "mlp_rank": 0}
    for name in calls:
        real = getattr(native, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(native, name, counted)
    return calls


def _exclude(rng, B, n_cols, gpu):
    lists = [rng.integers(0, n_cols, int(rng.integers(0, n_cols // 3))).tolist() for _ in range(B)]
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=gpu)
    return rowptr, torch.tensor(np.concatenate([np.asarray(x, np.int64) for x in lists]), dtype=torch.int32, device=gpu)


def test_top_k_items_ranks_content_rows_through_the_fused_kernel(gpu, mlp_calls):
    from deeprecommendation_amd import top_k_items
    m, prof, feat = _second_shape(gpu)
    m.set_content(prof, feat)
    rng = np.random.default_rng(2)
    users = torch.as_tensor(rng.integers(0, U, 64), device=gpu)
    exclude = _exclude(rng, 64, I, gpu)
    got = top_k_items(m, users, 20, exclude=exclude)
    assert mlp_calls["mlp_topk"] == 1
    _equal(got, top_k_items(m, users, 20, exclude=exclude, fused=False))
    _equal(got, top_k_items(m, users, 20, exclude=exclude, fused=False, block_bytes=7 * I * 20))     # several score blocks
    assert mlp_calls["mlp_topk"] == 1
    s, pos, n = got
    assert int(pos.max()) >= F and int(pos.max()) < I and bool((n == 20).all())      # the ranked list is the I items, not F columns
    with torch.no_grad():
        rows = m(prof[users.repeat_interleave(20)], feat[pos.reshape(-1)])
    assert_close(s.reshape(-1, 1), rows)
    seen = torch.zeros(64, I, dtype=torch.bool, device=gpu)
    seen[torch.repeat_interleave(torch.arange(64, device=gpu), exclude[0][1:] - exclude[0][:-1]), exclude[1].long()] = True
    assert not bool(seen.gather(1, pos).any())
    items = torch.as_tensor(rng.permutation(I)[:250], device=gpu)
    sub = top_k_items(m, users, 20, item_ids=items)
    assert mlp_calls["mlp_topk"] == 2
    _equal(sub, top_k_items(m, users, 20, item_ids=items, fused=False))
    assert bool(torch.isin(sub[1], items).all())
    with pytest.raises(ValueError):
        top_k_items(m, users, 20, profiles=(feat, None))


def test_rank_of_items_and_full_ranking_metrics(gpu, mlp_calls):
    from deeprecommendation_amd import eval_full_ranking, rank_of_items
    m, prof, feat = _second_shape(gpu)
    m.set_content(prof, feat)
    rng = np.random.default_rng(4)
    users = torch.as_tensor(rng.permutation(U)[:64], device=gpu)
    exclude = _exclude(rng, 64, I, gpu)
    cnt = rng.integers(1, 6, 64)
    trow = torch.tensor(np.concatenate([[0], np.cumsum(cnt)]), dtype=torch.int64, device=gpu)
    tcol = torch.tensor(np.concatenate([rng.choice(I, int(c), replace=False) for c in cnt]), dtype=torch.int32, device=gpu)
    rank, ranked = rank_of_items(m, users, (trow, tcol), exclude=exclude)
    assert mlp_calls["mlp_rank"] == 1
    _equal((rank, ranked), rank_of_items(m, users, (trow, tcol), exclude=exclude, fused=False))
    assert mlp_calls["mlp_rank"] == 1
    assert int(ranked.max()) <= I and int(ranked.max()) > F and int(rank.max()) >= F
    a = eval_full_ranking(m, users, (trow, tcol), exclude=exclude)
    b = eval_full_ranking(m, users, (trow, tcol), exclude=exclude, fused=False)
    assert a == b and a["users"] > 0


def _toy_provider(rng, n_users=U, n_items=I, width=F):
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    item_ids = np.arange(1, n_items + 1) * 3
    user_ids = (np.arange(1, n_users + 1) * 2)[rng.permutation(n_users)]            # provider order is not sorted order
    rated = [np.sort(rng.choice(item_ids, int(rng.integers(0, 40)), replace=False)) for _ in user_ids]
    ratings = [rng.integers(1, 11, len(r)) * 0.5 for r in rated]
    means = [float(r.mean()) if len(r) else 0.0 for r in ratings]
    feats = rng.standard_normal((n_items, width)).astype(np.float32)
    return SparseDynamicProvider(item_ids, feats, user_ids, rated, ratings, means), item_ids, user_ids


def test_providers_build_the_profiles_and_the_datasets_go_resident(gpu):
    import pandas as pd
    from deeprecommendation_amd import native
    from deeprecommendation_amd.content_providers.index_providers import ContentIndexProvider
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset
    from deeprecommendation_amd.neural_collaborative_filtering.eval import eval_model
    rng = np.random.default_rng(9)
    prov, item_ids, user_ids = _toy_provider(rng)
    table = prov.user_profiles(gpu)
    assert prov.user_profiles(gpu) is table and table.shape == (U, F) and table.dtype == torch.float32
    ref = profiles_loop(*prov.profile_csr(), prov.features.numpy())
    assert torch.equal(table.cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32))
    empty = [k for k, r in enumerate(prov.user_rated_items) if len(r) == 0]
    assert empty and not bool(table[empty].any())
    cp = ContentIndexProvider.from_dynamic(prov, gpu)
    prof, feat = cp.content(gpu)
    assert prof.is_cuda and feat.is_cuda and cp.get_item_feature_dim() == F
    assert torch.equal(prof[torch.from_numpy(cp.get_user_profile(user_ids)).to(gpu)], table) and torch.equal(feat.cpu(), prov.features)
    m, _, _ = _second_shape(gpu)
    m.set_content(prof, feat)
    n = 1500
    frame = pd.DataFrame({"userId": rng.choice(user_ids, n), "movieId": rng.choice(item_ids, n), "rating": rng.integers(1, 11, n) * 0.5})
    ds = FixedPointwiseDataset(frame, cp)
    fast = eval_model(m, ds, batch_size=256, device=gpu, resident=True)
    slow = eval_model(m, ds, batch_size=256, device=gpu, resident=False)
    assert np.array_equal(fast["predictions"], slow["predictions"]) and abs(fast["mse"] - slow["mse"]) <= 1e-12 * slow["mse"]
    with torch.no_grad():
        rows = m(prof[torch.from_numpy(cp.get_user_profile(frame["userId"].values)).to(gpu)],
                 feat[torch.from_numpy(cp.get_item_profile(frame["movieId"].values)).to(gpu)])
    assert_close(torch.as_tensor(np.asarray(fast["predictions"], dtype=np.float32)).reshape(-1, 1), rows)
    native.check_oob(gpu)


# ----------------------------------------------------------------------------- content-based baseline
def test_content_cosine_baseline_against_float64(gpu):
    from deeprecommendation_amd import content_cosine_ranks, content_cosine_top_k
    prof, feat, cos, order = cosine_case()
    ok = decided(cos, order)
    assert undecided_share(cos, order) <= 0.05           # what the seed leaves out for near-ties (float64 scores alone)
    users = torch.arange(COS_USERS, device=gpu)
    dp, df = torch.from_numpy(prof).to(gpu), torch.from_numpy(feat).to(gpu)
    s, pos, n = content_cosine_top_k(dp, df, users, COS_K)
    s, pos = s.cpu().numpy().astype(np.float64), pos.cpu().numpy()
    assert bool((n == COS_K).all())
    want = np.take_along_axis(cos, pos, axis=1)          # the float64 cosine of every returned (user, item)
    assert np.abs(s - want).max() <= COS_TOL
    assert not s[ZERO_USER].any() and np.array_equal(pos[ZERO_USER], np.arange(COS_K))
    live = np.arange(COS_USERS) != ZERO_USER
    assert np.array_equal(pos[live][ok[live]], order[:, :COS_K][live][ok[live]])
    # blocks of users, a subset of the items, an exclusion: the same scores for the same pairs
    items = torch.arange(COS_ITEMS - 1, -1, -2, device=gpu)
    s2, pos2, _ = content_cosine_top_k(dp, df, users[5:29], COS_K, item_ids=items, block_bytes=5 * items.numel() * 4)
    assert bool(torch.isin(pos2, items).all())
    assert np.abs(s2.cpu().numpy() - np.take_along_axis(cos[5:29], pos2.cpu().numpy(), axis=1)).max() <= COS_TOL
    excl = (torch.arange(0, 3 * COS_USERS + 1, 3, device=gpu), torch.from_numpy(order[:, :3].astype(np.int32)).reshape(-1).to(gpu))
    _, pos3, _ = content_cosine_top_k(dp, df, users, COS_K, exclude=excl)
    assert not bool((pos3[:, :, None].cpu() == torch.from_numpy(order[:, None, :3])).any())
    # the ranks twin: a decided slot's item holds that slot
    tcol = torch.from_numpy(order[:, :COS_K].astype(np.int32)).reshape(-1).to(gpu)
    trow = torch.arange(0, COS_K * COS_USERS + 1, COS_K, device=gpu)
    rank, ranked = content_cosine_ranks(dp, df, users, (trow, tcol))
    rank = rank.cpu().numpy().reshape(COS_USERS, COS_K)
    assert bool((ranked == COS_ITEMS).all())
    assert np.array_equal(rank[live][ok[live]], np.broadcast_to(np.arange(COS_K), rank.shape)[live][ok[live]])
