"""GPU: AttentionNCF in the ranking front end — catalogue_scores (logit-table route and pair route), top_k_items, rank_of_items and
eval_full_ranking with ``profiles=`` — against the oracle's attention_ncf_forward on the dense expanded inputs and against host
restatements of the ranking contract.

A small model (item_dim 40, item_emb = user_emb = 64, MLP [256, 128]) in its three attention forms (att_dense = 32, att_dense = None,
cosine), a catalogue of 150 items and 12 users with rated sets of 0, 1, 5, 64, 65 and 120 items, ratings of both signs; every user
with a rated set also rated two items with exactly their centre value, which the provider drops."""
import numpy as np
import pytest
import torch

from oracle import ncf_oracle as O
from rank_ref import csr, rank_oracle
from test_gpu_basic import assert_close

pytestmark = pytest.mark.gpu

I_CAT, F_DIM = 150, 40
SET_SIZES = (0, 1, 5, 64, 65, 120, 120, 65, 64, 5, 1, 0)
FORMS = {"mlp": dict(att_dense=32), "linear": dict(att_dense=None), "cos": dict(att_dense=None, use_cos_sim_instead=True)}


def _provider():
    from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider
    rng = np.random.default_rng(2025)
    feats = (rng.random((I_CAT, F_DIM)) < 0.2).astype(np.float32) * rng.random((I_CAT, F_DIM)).astype(np.float32)
    rated, ratings = [], []
    for n in SET_SIZES:
        items = np.sort(rng.permutation(I_CAT)[:n + (2 if n else 0)]) + 1
        r = rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 3.5, 4.0, 4.5, 5.0], len(items))     # centre 2.5: both signs, never 0 ...
        if n:
            r[rng.permutation(len(items))[:2]] = 2.5                                  # ... but for two items, which are dropped
        rated.append(items)
        ratings.append(r)
    means = np.full(len(SET_SIZES), 2.5)
    return SparseDynamicProvider(np.arange(1, I_CAT + 1), feats, np.arange(len(SET_SIZES)), rated, ratings, means, sparse=True)


@pytest.fixture(scope="module")
def world(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import SparseRatings
    prov = _provider()
    st = prov.device_state(gpu)
    ratings = SparseRatings(st.rowptr, st.col, st.val, st.num_items)
    lens = (st.rowptr[1:] - st.rowptr[:-1]).tolist()
    assert lens == list(SET_SIZES) and bool((st.val > 0).any()) and bool((st.val < 0).any())
    return dict(prov=prov, state=st, feats=st.features, ratings=ratings, dense=ratings.to_dense(ratings.val).cpu())


@pytest.fixture(scope="module")
def models(gpu):
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    out = {}
    for k, (name, kw) in enumerate(FORMS.items()):
        torch.manual_seed(100 + k)
        out[name] = AttentionNCF(item_dim=F_DIM, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128], **kw).eval().to(gpu)
    return out


@pytest.fixture(scope="module")
def reference(world, models):
    """The oracle's scores (U, I_cat) per form: every user against the whole catalogue, dense expanded inputs, on the CPU."""
    feats, dense = world["feats"].cpu(), world["dense"]
    U = dense.shape[0]
    ref = {}
    for name, m in models.items():
        state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        with torch.no_grad():
            ref[name] = O.attention_ncf_forward(state, feats.repeat(U, 1), feats, dense.repeat_interleave(I_CAT, dim=0),
                                                use_cos_sim_instead=name == "cos").view(U, I_CAT)
    return ref


def _users(gpu, n=len(SET_SIZES)):
    return torch.arange(n, dtype=torch.int64, device=gpu)


def test_top_k_items_takes_an_attention_model(gpu, world, models):
    """Fails on a tree without the feature: top_k_items had no route for an AttentionNCF."""
    from deeprecommendation_amd import top_k_items
    s, pos, n = top_k_items(models["mlp"], _users(gpu), 10, profiles=(world["feats"], world["ratings"]))
    assert s.shape == (len(SET_SIZES), 10) and pos.dtype == torch.int64 and n.tolist() == [10] * len(SET_SIZES)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("table", [True, False])
def test_catalogue_scores_match_the_oracle(gpu, world, models, reference, form, table):
    from deeprecommendation_amd import native
    m = models[form]
    got = m.catalogue_scores(world["feats"], world["ratings"], _users(gpu), table=table)
    native.check_oob(gpu)
    assert got.shape == (len(SET_SIZES), I_CAT) and got.dtype == torch.float32
    assert_close(got, reference[form])
    # a shuffled subset of the catalogue, users repeated and out of order
    items = torch.tensor(np.random.default_rng(3).permutation(I_CAT)[:70], device=gpu)
    users = torch.tensor([7, 3, 3, 0, 11, 5], device=gpu)
    sub = m.catalogue_scores(world["feats"], world["ratings"], users, item_ids=items, table=table)
    assert_close(sub, reference[form][users.cpu()][:, items.cpu()])
    assert torch.equal(sub, got[users][:, items])                    # the same bits as the full call's entries


def _host_topk(scores, k, lists):
    """top_k_items' contract on the host: stable descending sort of the non-excluded columns; -1 / -inf past the count."""
    S = scores.cpu().clone()
    U, I = S.shape
    out_s = torch.full((U, k), -float("inf"))
    out_i = torch.full((U, k), -1, dtype=torch.int64)
    cnt = torch.zeros(U, dtype=torch.int32)
    for r in range(U):
        keep = torch.ones(I, dtype=torch.bool)
        if lists is not None:
            ids = [c for c in lists[r] if 0 <= c < I]
            if ids:
                keep[ids] = False
        cols = keep.nonzero().view(-1)
        v, order = torch.sort(S[r, cols], descending=True, stable=True)
        n = min(k, cols.numel())
        out_s[r, :n], out_i[r, :n], cnt[r] = v[:n], cols[order[:n]], n
    return out_s, out_i, cnt


@pytest.mark.parametrize("form,fused", [("mlp", True), ("mlp", False), ("linear", None), ("cos", True)])
def test_top_k_items_is_topk_rows_of_catalogue_scores(gpu, world, models, form, fused):
    from deeprecommendation_amd import native, rated_exclusion, top_k_items
    m, feats, ratings = models[form], world["feats"], world["ratings"]
    users = torch.tensor([4, 0, 5, 9, 2, 2, 11, 6], dtype=torch.int64, device=gpu)
    items = torch.tensor(np.random.default_rng(5).permutation(I_CAT)[:90], dtype=torch.int64, device=gpu)
    excl = rated_exclusion(ratings, users)
    rp, rc = ratings.rowptr.cpu(), ratings.col.cpu()
    rated = [rc[int(rp[u]):int(rp[u + 1])].tolist() for u in users.tolist()]
    assert excl[0].dtype == torch.int64 and excl[1].dtype == torch.int32
    assert [excl[1][int(a):int(b)].tolist() for a, b in zip(excl[0][:-1].tolist(), excl[0][1:].tolist())] == rated
    full = m.catalogue_scores(feats, ratings, users, table=fused)
    for k in (1, 10, 150):
        for exclude, lists in ((None, None), (excl, rated)):
            s, pos, n = top_k_items(m, users, k, exclude=exclude, profiles=(feats, ratings), fused=fused)
            ws, wi, wn = native.topk_rows(full, k, exclude)
            assert torch.equal(s, ws) and torch.equal(pos, wi.to(torch.int64)) and torch.equal(n, wn)
            hs, hi, hn = _host_topk(full, k, lists)
            assert torch.equal(s.cpu(), hs) and torch.equal(pos.cpu(), hi) and torch.equal(n.cpu(), hn)
            want_n = [min(k, I_CAT - len(set(l))) for l in lists] if lists else [min(k, I_CAT)] * len(rated)
            assert n.tolist() == want_n
    # item_ids a shuffled subset: columns of the list, positions of the catalogue returned; exclude names columns of the list
    sub = m.catalogue_scores(feats, ratings, users, item_ids=items, table=fused)
    col_lists = [list(range(r, 90, 7)) for r in range(users.numel())]
    s, pos, n = top_k_items(m, users, 10, item_ids=items, exclude=csr(col_lists, gpu), profiles=(feats, ratings), fused=fused)
    hs, hi, hn = _host_topk(sub, 10, col_lists)
    assert torch.equal(s.cpu(), hs) and torch.equal(pos.cpu(), items.cpu()[hi]) and torch.equal(n.cpu(), hn)
    native.check_oob(gpu)


@pytest.mark.parametrize("form,fused", [("mlp", None), ("cos", False)])
def test_ranks_and_metrics(gpu, world, models, form, fused):
    from deeprecommendation_amd import eval_full_ranking, rank_of_items, ranking_metrics, rated_exclusion
    m, feats, ratings = models[form], world["feats"], world["ratings"]
    users = _users(gpu)
    rng = np.random.default_rng(17)
    targets = [rng.permutation(I_CAT)[:int(rng.integers(0, 6))].tolist() for _ in range(users.numel())]
    targets[3] = rng.permutation(I_CAT)[:140].tolist()              # more targets than any fused rank kernel takes: no cap on this route
    excl = rated_exclusion(ratings, users)
    rp, rc = ratings.rowptr.cpu(), ratings.col.cpu()
    rated = [rc[int(rp[u]):int(rp[u + 1])].tolist() for u in range(users.numel())]
    full = m.catalogue_scores(feats, ratings, users, table=fused)
    tg = csr(targets, gpu)
    rank, ranked = rank_of_items(m, users, tg, exclude=excl, profiles=(feats, ratings), fused=fused)
    want_rank, want_ranked = rank_oracle(full, rated, targets)
    assert torch.equal(rank.cpu(), want_rank) and torch.equal(ranked.cpu(), want_ranked)
    got = eval_full_ranking(m, users, tg, exclude=excl, profiles=(feats, ratings), fused=fused)
    ref = ranking_metrics(want_rank, tg[0].cpu(), want_ranked)
    assert set(got) == set(ref)
    for k in ref:                                                   # float64 on the device against float64 on the host
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])


def test_user_blocks_give_the_same_bits(gpu, world, models):
    from deeprecommendation_amd import top_k_items
    m, feats, ratings = models["mlp"], world["feats"], world["ratings"]
    users = _users(gpu)
    for table in (True, False):
        one = m.catalogue_scores(feats, ratings, users, table=table)
        per_pair = 4 * 64 + 4 + 8
        blocks = list(m.catalogue_score_blocks(feats, ratings, users, table=table, block_bytes=5 * I_CAT * per_pair))
        assert [(a, b) for a, b, _ in blocks] == [(0, 5), (5, 10), (10, 12)]
        assert torch.equal(torch.cat([s for _, _, s in blocks]), one)
        a = top_k_items(m, users, 10, profiles=(feats, ratings), fused=table)
        b = top_k_items(m, users, 10, profiles=(feats, ratings), fused=table, block_bytes=5 * I_CAT * per_pair)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_table_is_built_once_per_weight_version(gpu, world, models, monkeypatch):
    from deeprecommendation_amd import native
    m, feats, ratings = models["mlp"], world["feats"], world["ratings"]
    calls = []
    real = native.attn_logits
    monkeypatch.setattr(native, "attn_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        m.MLP[0].bias.add_(0.0)                                     # a new weight version: whatever was cached is dropped
    first = m.catalogue_scores(feats, ratings, _users(gpu), table=True)
    again = m.catalogue_scores(feats, ratings, _users(gpu)[:4], table=True)
    assert len(calls) == 1 and torch.equal(again, first[:4])
    with torch.no_grad():
        m.AttentionNet[0].weight.mul_(1.0)                          # an in-place edit of a weight (same values, new version)
    third = m.catalogue_scores(feats, ratings, _users(gpu), table=True)
    assert len(calls) == 2 and torch.equal(third, first)
    m.catalogue_scores(feats, ratings, _users(gpu), table=False)
    assert len(calls) == 2                                          # the pair route needs no table


def test_a_width_the_cross_kernel_refuses_takes_the_pair_route(gpu, world, monkeypatch):
    from deeprecommendation_amd import native, top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(9)
    m = AttentionNCF(item_dim=F_DIM, item_emb=64, user_emb=48, att_dense=32, mlp_dense_layers=[256, 128]).eval().to(gpu)
    feats, ratings, users = world["feats"], world["ratings"], _users(gpu)
    assert not native.attn_cross_supported(48) and not m.cross_route(I_CAT) and not m.cross_route(I_CAT, False)
    calls = []
    real = native.attn_cross
    monkeypatch.setattr(native, "attn_cross", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    s, pos, n = top_k_items(m, users, 5, profiles=(feats, ratings))
    assert not calls and torch.equal(s, native.topk_rows(m.catalogue_scores(feats, ratings, users, table=False), 5)[0])
    with pytest.raises(ValueError, match="user_emb = 48"):
        top_k_items(m, users, 5, profiles=(feats, ratings), fused=True)
    with pytest.raises(ValueError, match="user_emb = 48"):
        m.catalogue_scores(feats, ratings, users, table=True)


def test_a_provider_device_state_is_taken_as_it_is(gpu, world, models):
    from deeprecommendation_amd import rated_exclusion, top_k_items
    st, m = world["state"], models["linear"]
    users = _users(gpu, st.rowptr.numel() - 1)                      # the whole user base
    a = top_k_items(m, users, 10, profiles=(st.features, st), exclude=rated_exclusion(st, users))
    b = top_k_items(m, users, 10, profiles=(world["feats"], world["ratings"]), exclude=rated_exclusion(world["ratings"], users))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rp, rc = st.rowptr.cpu(), st.col.cpu()
    for u in range(users.numel()):                                  # nothing a user rated is recommended to them
        assert not set(a[1][u, :int(a[2][u])].tolist()) & set(rc[int(rp[u]):int(rp[u + 1])].tolist())
