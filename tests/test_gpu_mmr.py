"""GPU: ncf_mmr_rerank against the three restatements of THE CONTRACT in tests/mmr_ref.py — bit for bit against the order-free loop
on exactly representable inputs (ties everywhere: the comparator is what is tested) and against the fp32 emulator on float inputs,
and within the near-tie rule against the float64 twin; out-of-range positions are refused, not read through; two launches give the
same bits; diversify_top_k / item_vectors / the two metrics on small models."""
import numpy as np
import pytest
import torch

import mmr_ref as R

pytestmark = pytest.mark.gpu


def _launch(gpu, case):
    from deeprecommendation_amd import native
    vec = torch.from_numpy(case["vec"]).to(gpu)[:, :case["D"]]             # rows of ldv floats: a column slice
    count = None if case["count"] is None else torch.from_numpy(case["count"]).to(gpu)
    slot, value, cnt = native.mmr_rerank(vec, torch.from_numpy(case["score"]).to(gpu), torch.from_numpy(case["pos"]).to(gpu), count,
                                         case["K"], case["lam"], bool(case["normalize"]))
    assert slot.dtype == torch.int32 and value.dtype == torch.float32 and cnt.dtype == torch.int32
    return slot.cpu().numpy(), value.cpu().numpy(), cnt.cpu().numpy()


def _assert_bits(got, want, name):
    for g, w, what in zip(got, want, ("slot", "value", "count")):
        assert g.shape == w.shape, (name, what)
        same = np.array_equal(g.view(np.int32), w.view(np.int32))
        if not same:
            b = int(np.argwhere((g.view(np.int32) != w.view(np.int32)).reshape(g.shape[0], -1).any(axis=1))[0, 0])
            pytest.fail(f"{name}: {what} differs first at user {b}: got {g[b]}, want {w[b]}")


@pytest.mark.parametrize("N", R.EXACT_N)
def test_exact_cases_bit_for_bit_against_the_order_free_loop(gpu, N):
    from deeprecommendation_amd import native
    cases = [c for c in R.exact_cases() if c["score"].shape[1] == N]
    assert len(cases) >= 5
    for case in cases:
        _assert_bits(_launch(gpu, case), R.rerank(case, "exact"), case["name"])
    native.check_oob(gpu)                         # -1 and dead scores raise nothing


@pytest.mark.parametrize("i", range(12))
def test_float_cases_bit_for_bit_against_the_fp32_emulator(gpu, i):
    from deeprecommendation_amd import native
    case = R.float_cases()[i]
    _assert_bits(_launch(gpu, case), R.rerank(case, "f32"), case["name"])
    native.check_oob(gpu)


@pytest.mark.parametrize("i", range(3))
def test_float_cases_stay_with_the_float64_twin(gpu, i):
    case = R.twin_cases()[i]
    slot, _, cnt = _launch(gpu, case)
    left_out, wrong = R.twin_verdict(i, slot)
    print(f"{case['name']}: {len(left_out)} of {slot.shape[0]} users left out, {len(wrong)} beyond the margin of {R.TWIN_MARGIN}")
    assert (cnt == case["K"]).all() and not wrong and len(left_out) <= R.TWIN_CAP * slot.shape[0]


def test_out_of_range_position_is_refused_and_flagged(gpu):
    from deeprecommendation_amd import native
    clean = R.float_cases()[6]                    # N 128, D 64, K 20, 40 pools
    native.check_oob(gpu)
    before = _launch(gpu, clean)
    score, pos = clean["score"].copy(), clean["pos"].copy()
    score[17, 5], pos[17, 5] = 2.0, clean["n_items"]              # the most relevant slot of pool 17 points one past the table
    score[17, 9], pos[17, 9] = 1.5, -7
    case = dict(clean, score=score, pos=pos)
    got = _launch(gpu, case)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                         # raised once, cleared
    want = R.rerank(case, "f32")
    assert want[3] and 5 not in got[0][17] and 9 not in got[0][17]
    _assert_bits(got, want[:3], "out of range")
    others = np.arange(40) != 17
    for g, b in zip(got, before):
        assert np.array_equal(g[others].view(np.int32), b[others].view(np.int32))
    native.check_oob(gpu)


def test_two_launches_give_the_same_bits(gpu):
    for case in (R.float_cases()[8], R.float_cases()[9]):            # staged, and rows past the LDS image
        a, b = _launch(gpu, case), _launch(gpu, case)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- front end
def _pool_case(scores, positions, counts, vectors, k, lam, normalize):
    return dict(vec=vectors.cpu().numpy(), D=vectors.shape[1], score=scores.cpu().numpy(), pos=positions.cpu().numpy(),
                count=counts.cpu().numpy(), K=k, lam=lam, normalize=normalize, n_items=vectors.shape[0])


def _check_front_end(gpu, pool, vectors, pure):
    from deeprecommendation_amd import diversify_top_k, native
    s, p, c = pool
    norms = vectors.double().norm(dim=1)
    assert vectors.dtype == torch.float32 and float((norms - 1).abs().max()) <= 1e-6
    ds, dp, dc, dv = diversify_top_k(s, p, c, vectors, 10, lam=0.5)
    slot, value, cnt, _ = R.rerank(_pool_case(s, p, c, vectors, 10, 0.5, 1), "f32")
    assert ds.shape == dp.shape == dv.shape == (s.shape[0], 10) and dp.dtype == torch.int64 and dc.dtype == torch.int32
    assert np.array_equal(dc.cpu().numpy(), cnt) and np.array_equal(dv.cpu().numpy().view(np.int32), value.view(np.int32))
    rows = np.arange(s.shape[0])[:, None]
    picked = slot >= 0
    want_p = np.where(picked, p.cpu().numpy()[rows, np.maximum(slot, 0)], -1)
    want_s = np.where(picked, s.cpu().numpy()[rows, np.maximum(slot, 0)], -np.inf).astype(np.float32)
    assert np.array_equal(dp.cpu().numpy(), want_p) and np.array_equal(ds.cpu().numpy().view(np.int32), want_s.view(np.int32))
    for x, y in zip(diversify_top_k(s, p, c, vectors, 10, lam=1, normalize=None)[:3], pure):
        assert x.dtype == y.dtype and torch.equal(x, y)
    native.check_oob(gpu)


def test_diversify_an_mf_pool(gpu):
    from deeprecommendation_amd import item_vectors, top_k_items
    from deeprecommendation_amd.neural_collaborative_filtering.models.mf import MF
    torch.manual_seed(3)
    m = MF(item_dim=150, user_dim=40, item_emb=32, user_emb=32).eval().to(gpu)
    users = torch.arange(40, device=gpu)
    vectors = item_vectors(m)
    assert vectors.shape == (150, 32)
    _check_front_end(gpu, top_k_items(m, users, 64), vectors, top_k_items(m, users, 10))
    small = MF(item_dim=40, user_dim=8, item_emb=16, user_emb=16).eval().to(gpu)       # fewer items than slots: -1 padding in the pool
    _check_front_end(gpu, top_k_items(small, users[:8], 64), item_vectors(small), top_k_items(small, users[:8], 10))


def test_diversify_a_graph_dot_pool(gpu):
    from deeprecommendation_amd import item_vectors, seen_items, top_k_items
    from test_gpu_recommend_graph import N_ITEMS, N_USERS, _graph_model
    m, _, graph, _ = _graph_model(gpu, True, False, True, seed=9)
    users = torch.arange(N_ITEMS, N_ITEMS + N_USERS, device=gpu)
    exclude = seen_items(graph, users)
    vectors = item_vectors(m, graph=graph)
    assert vectors.shape[0] == N_ITEMS
    _check_front_end(gpu, top_k_items(m, users, 64, graph=graph, exclude=exclude), vectors,
                     top_k_items(m, users, 10, graph=graph, exclude=exclude))


def test_item_vectors_of_an_attention_model_are_unit_rows(gpu):
    from deeprecommendation_amd import item_vectors
    from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    torch.manual_seed(5)
    m = AttentionNCF(item_dim=24, item_emb=32, user_emb=32, att_dense=16, mlp_dense_layers=[16]).eval().to(gpu)
    feats = torch.randn(70, 24, device=gpu)
    vectors = item_vectors(m, item_features=feats)
    li = m.ItemEmbeddings[0]
    with torch.no_grad():
        want = torch.nn.functional.normalize(feats.double() @ li.weight.double().t() + li.bias.double(), dim=1)
    assert vectors.shape == (70, 32) and float((vectors.double() - want).abs().max()) <= 1e-5
    assert float((vectors.double().norm(dim=1) - 1).abs().max()) <= 1e-6


def test_low_lambda_raises_diversity_and_coverage_on_four_clusters(gpu):
    """Four tight clusters, every user's relevance favouring one of them: the lists at lam = 0.3 are strictly more diverse on average
    than at lam = 1 (checked with the reference first), and reach more of the catalogue."""
    from deeprecommendation_amd import catalogue_coverage, diversify_top_k, intra_list_diversity
    vec, score, pos, cluster = R.cluster_fixture()
    rng = np.random.default_rng(13)
    B, N = 12, vec.shape[0]
    scores = np.stack([(1.0 - 0.1 * ((cluster + b) % 4) + 0.05 * rng.uniform(size=N)) for b in range(B)]).astype(np.float32)
    positions = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64)
    scores = np.take_along_axis(scores, positions, axis=1)                        # the score of the item in the slot
    counts = np.full(B, N, dtype=np.int32)
    ild = {}
    for lam in (0.3, 1.0):
        case = dict(vec=vec, D=vec.shape[1], score=scores, pos=positions, count=counts, K=8, lam=lam, normalize=1)
        slot, _, cnt, _ = R.rerank(case, "f32")
        ild[lam] = R.ild_ref(np.take_along_axis(positions, slot.astype(np.int64), axis=1), cnt, vec).mean()
    assert ild[0.3] > ild[1.0]
    V = torch.from_numpy(vec).to(gpu)
    got = {}
    for lam in (0.3, 1.0):
        _, p, c, _ = diversify_top_k(torch.from_numpy(scores).to(gpu), torch.from_numpy(positions).to(gpu), torch.from_numpy(counts).to(gpu),
                                     V, 8, lam=lam)
        d = intra_list_diversity(p, c, V)
        want = R.ild_ref(p.cpu().numpy(), c.cpu().numpy(), vec)
        assert d.dtype == torch.float32 and (np.abs(d.cpu().numpy() - want) <= 1e-5 * np.abs(want) + 1e-6).all()
        cov = catalogue_coverage(p, c, N)
        assert float(cov) == R.coverage_ref(p.cpu().numpy(), c.cpu().numpy(), N)
        got[lam] = (float(d.mean()), float(cov))
    assert got[0.3][0] > got[1.0][0] and abs(got[0.3][0] - ild[0.3]) <= 1e-5 and abs(got[1.0][0] - ild[1.0]) <= 1e-5
