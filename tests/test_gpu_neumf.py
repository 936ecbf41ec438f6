"""GPU tests of NeuMF: the pair scorer bit for bit against the fused MLP scorer plus the restated GMF term, the model's eval forward,
the full-catalogue top-K and ranks against score-then-select on every plan the cases claim, and a training step."""
import copy

import numpy as np
import pytest
import torch

import fused_forms_ref as F
import neumf_ref as R
import rank_forms_ref as K

pytestmark = pytest.mark.gpu

# (K0, N1, N2) with the split (EA, EB) of the concat
TOWERS = {(64, 128, 0): (24, 40), (128, 128, 64): (64, 64), (128, 256, 128): (64, 64)}
N_USERS, N_ITEMS = 211, 157


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _hidden(tower):
    return [n for n in tower[1:] if n]


def _random_case(tower, D, seed):
    """CPU fp32 tables and weights of one tower with a D-wide GMF branch: weights = [W1, (W2,) wl], biases = [b1, (b2,) bl]."""
    g = torch.Generator().manual_seed(seed)
    EA, EB = TOWERS[tower]
    ws, bs = F.random_mlp(g, [tower[0]] + _hidden(tower) + [1])
    tabs = [torch.randn(n, e, generator=g) for n, e in ((N_USERS, EA), (N_ITEMS, EB), (N_USERS, D), (N_ITEMS, D))]
    w = torch.randn(D, generator=g)
    return tabs, ws, bs, w


def _reference(native, dev, tabs, ws, bs, w, users, items):
    """The contract's value from its parts: s_mlp = the fused scorer with the blob re-packed with a zero last bias (on the device), g by
    neumf_ref and the two final sums on the host.  Returns (score (B,) fp32 tensor, the device tensors and the packed tower)."""
    d = [t.to(dev) for t in tabs]
    packed0 = native.PackedMLP([x.to(dev) for x in ws], [x.to(dev) for x in bs[:-1]] + [torch.zeros(1, device=dev)])
    s_mlp = native.score_fused(d[0], users.to(dev), d[1], items.to(dev), packed0).cpu().numpy().reshape(-1)
    g = R.gmf_fp32(w.numpy(), R.gather_rows(tabs[2], users).numpy(), R.gather_rows(tabs[3], items).numpy())
    ref = torch.from_numpy(R.finish_fp32(s_mlp, g, bs[-1].numpy()[0]))
    packed = native.PackedMLP([x.to(dev) for x in ws], [x.to(dev) for x in bs])
    return ref, d, packed


@pytest.mark.parametrize("B", [1, 33, 257])
@pytest.mark.parametrize("D", [8, 24, 128])
@pytest.mark.parametrize("tower", list(TOWERS))
def test_pair_scorer_has_the_contract_bits(native, gpu, tower, D, B):
    """One lane, a ragged second tile, a ragged third workgroup; random fp32 data."""
    tabs, ws, bs, w = _random_case(tower, D, 1000 * D + B + tower[1])
    EA, EB = TOWERS[tower]
    g = torch.Generator().manual_seed(B)
    users, items = torch.randint(0, N_USERS, (B,), generator=g), torch.randint(0, N_ITEMS, (B,), generator=g)
    ref, d, packed = _reference(native, gpu, tabs, ws, bs, w, users, items)
    assert native.neumf_supported(packed, EA, EB, D)
    out = native.neumf_score(d[0], users.to(gpu), d[1], items.to(gpu), d[2], d[3], packed, w.to(gpu))
    assert out.shape == (B, 1)
    F.assert_same_bits(out, ref, f"{tower} D={D} B={B}")
    native.check_oob(gpu)
    R.assert_close(out, R.forward_f64(*tabs, ws, bs, w, users, items), "against float64")


@pytest.mark.parametrize("side", ["user", "item"])
def test_out_of_range_id_reads_zero_rows_and_sets_the_flag(native, gpu, side):
    tower, D, B = (128, 128, 64), 24, 33
    tabs, ws, bs, w = _random_case(tower, D, 77)
    g = torch.Generator().manual_seed(3)
    users, items = torch.randint(0, N_USERS, (B,), generator=g), torch.randint(0, N_ITEMS, (B,), generator=g)
    if side == "user":
        users[5], users[17] = N_USERS, -1
    else:
        items[0], items[32] = -7, N_ITEMS + 3
    ref, d, packed = _reference(native, gpu, tabs, ws, bs, w, users, items)
    with pytest.raises(IndexError):                  # the fused scorer of the reference met the id too
        native.check_oob(gpu)
    out = native.neumf_score(d[0], users.to(gpu), d[1], items.to(gpu), d[2], d[3], packed, w.to(gpu))
    F.assert_same_bits(out, ref, side)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    native.check_oob(gpu)                            # read and cleared
    R.assert_close(out, R.forward_f64(*tabs, ws, bs, w, users, items), "zero rows, float64")


@pytest.mark.parametrize("tower", list(TOWERS))
def test_pair_scorer_is_exact_on_integer_data(native, gpu, tower):
    """Small integers in fp32: every partial sum is exact in any order, so the float64 forward is the expected score bit for bit."""
    D, B = 24, 257
    EA, EB = TOWERS[tower]
    g = torch.Generator().manual_seed(tower[1] + tower[2])
    ta, tb, ws, bs = F.int_case(g, EA, EB, _hidden(tower), N_USERS, N_ITEMS)
    gu, gi = F._ints(g, (N_USERS, D), 3), F._ints(g, (N_ITEMS, D), 3)
    w = F._ints(g, (D,), 2)
    users, items = torch.randint(0, N_USERS, (B,), generator=g), torch.randint(0, N_ITEMS, (B,), generator=g)
    assert F.int_margin(ta, tb, users, items, ws, bs) + 18 * D + 3 < 2 ** 24
    ref = R.forward_f64(ta, tb, gu, gi, ws, bs, w, users, items)
    packed = native.PackedMLP([x.to(gpu) for x in ws], [x.to(gpu) for x in bs])
    out = native.neumf_score(ta.to(gpu), users.to(gpu), tb.to(gpu), items.to(gpu), gu.to(gpu), gi.to(gpu), packed, w.to(gpu))
    F.assert_same_bits(out, (ref + 0.0).float(), str(tower))


def test_refusals_of_the_wrappers(native, gpu):
    tabs, ws, bs, w = _random_case((64, 128, 0), 8, 5)
    d = [t.to(gpu) for t in tabs]
    packed = native.PackedMLP([x.to(gpu) for x in ws], [x.to(gpu) for x in bs])
    u, i = torch.zeros(4, dtype=torch.int64, device=gpu), torch.zeros(4, dtype=torch.int64, device=gpu)
    assert not native.neumf_supported(packed, 24, 40, 12) and not native.neumf_supported(packed, 24, 40, 136)
    assert not native.neumf_supported(packed, 20, 44, 8)
    with pytest.raises(native.NativeError) as e:
        native.neumf_score(d[0], u, d[1], i, torch.zeros(N_USERS, 12, device=gpu), torch.zeros(N_ITEMS, 12, device=gpu), packed,
                           torch.zeros(12, device=gpu))
    assert e.value.code == native.NCF_EUNSUPPORTED
    with pytest.raises(ValueError, match="rows of its side"):
        native.neumf_score(d[0], u, d[1], i, d[2][:-1], d[3], packed, w.to(gpu))
    with pytest.raises(ValueError, match="w has"):
        native.neumf_score(d[0], u, d[1], i, d[2], d[3], packed, torch.zeros(16, device=gpu))
    with pytest.raises(RuntimeError, match="GPU"):
        native.neumf_score(d[0], u, d[1], i, d[2].cpu(), d[3], packed, w.to(gpu))
    with pytest.raises(native.NativeError) as e:
        native.neumf_topk(d[0], None, d[1], None, d[2], d[3], packed, w.to(gpu), 129)
    assert e.value.code == native.NCF_EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------ the model
def _neumf(gpu, seed=0, **kw):
    from deeprecommendation_amd.neural_collaborative_filtering.models.neumf import NeuMF
    torch.manual_seed(seed)
    return NeuMF(item_dim=N_ITEMS, user_dim=N_USERS, **kw).to(gpu)


def _model_f64(m, users, items):
    lins = [x for x in m.MLP if isinstance(x, torch.nn.Linear)]
    D = m.mf_dim
    tab = lambda lin: (lin.weight.detach().double().t() + lin.bias.detach().double()).cpu()
    pw = m.predict.weight.detach().cpu()
    return R.forward_f64(tab(m.user_embeddings[0]), tab(m.item_embeddings[0]), tab(m.mf_user_embeddings[0]), tab(m.mf_item_embeddings[0]),
                         [l.weight for l in lins] + [pw[:, D:]], [l.bias for l in lins] + [m.predict.bias], pw[0, :D], users, items)


def test_eval_forward_is_the_kernel_on_the_models_tables(native, gpu):
    m = _neumf(gpu).eval()                             # the defaults: the (128, 128, 64) instance, D = 32
    g = torch.Generator().manual_seed(9)
    users, items = torch.randint(0, N_USERS, (257,), generator=g).to(gpu), torch.randint(0, N_ITEMS, (257,), generator=g).to(gpu)
    ops = m.kernel_operands()
    assert ops is not None
    with torch.no_grad():
        out = m(users, items)
    tabU, tabI, gmfU, gmfI, packed, w = ops
    F.assert_same_bits(out, native.neumf_score(tabU, users, tabI, items, gmfU, gmfI, packed, w), "model")
    R.assert_close(out, _model_f64(m, users.cpu(), items.cpu()), "model against float64")
    with torch.no_grad():
        m.predict.bias.add_(1.0)                       # an optimiser's in-place update: the packed tower of the old version is dropped
        R.assert_close(m(users, items), _model_f64(m, users.cpu(), items.cpu()), "after an update")


@pytest.mark.parametrize("kw", [dict(mf_dim=12), dict(mf_dim=8, mlp_dense_layers=[96]), dict(mf_dim=8, mlp_dense_layers=[64, 32, 16])])
def test_shapes_without_a_kernel_fall_back_to_torch_ops(native, gpu, kw):
    m = _neumf(gpu, 1, **kw).eval()
    assert m.kernel_operands() is None
    g = torch.Generator().manual_seed(2)
    users, items = torch.randint(0, N_USERS, (257,), generator=g).to(gpu), torch.randint(0, N_ITEMS, (257,), generator=g).to(gpu)
    with torch.no_grad():
        out = m(users, items)
    assert out.shape == (257, 1) and not out.requires_grad
    R.assert_close(out, _model_f64(m, users.cpu(), items.cpu()), str(kw))


# ------------------------------------------------------------------------------------------------------------------ ranking
D_RANK = 24
_CASE = {}


def _ranking_case(native, gpu, rows, cols, tile):
    """int_mlp's data at instance MAIN with integer GMF tables, and the (rows, cols) matrix of the pair scorer's scores: computed
    once per shape and shared, never changed."""
    key = (rows, cols, tile)
    if key not in _CASE:
        m = K.int_mlp(K.MAIN, cols, tile, rows)
        ws, bs = K.mlp_weights(m, True, gpu)
        g = torch.Generator().manual_seed(rows + cols)
        tabU, tabI = m["users"].float().to(gpu), m["items"].float().to(gpu)
        gmfU, gmfI = F._ints(g, (rows, D_RANK), 3).to(gpu), F._ints(g, (cols, D_RANK), 3).to(gpu)
        w = F._ints(g, (D_RANK,), 2).to(gpu)
        packed = native.PackedMLP(ws, bs)
        u = torch.arange(rows, device=gpu).repeat_interleave(cols)
        i = torch.arange(cols, device=gpu).repeat(rows)
        scores = native.neumf_score(tabU, u, tabI, i, gmfU, gmfI, packed, w).view(rows, cols)
        assert int(torch.isnan(scores[:, K.NAN_ITEM(cols)]).sum()) == rows      # the all-NaN column is there
        _CASE[key] = (tabU, tabI, gmfU, gmfI, packed, w, scores)
    return _CASE[key]


def _shape(tile):
    """(rows, cols) of rank_forms_ref's MLP cases at MAIN for a tile; tile 32 is the smallest shape: four ranges, the last ragged."""
    if tile == 32:
        return 3, 100
    c = K.select(entry="mlp_topk", inst=K.MAIN, tile=tile)[0]
    return c["rows"], c["cols"]


@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("tile,k", [(32, 1), (32, 10), (32, 128), (1024, 10), (1024, 128), (8192, 1), (8192, 10)])
def test_topk_is_score_then_select(native, gpu, tile, k, excl):
    assert tile == 32 or tile in K.MLP_MULTI_TILES
    rows, cols = _shape(tile)
    assert native.ranking_plan("mlp_topk", rows, cols, k)[:2] == (tile, -(-cols // tile))
    tabU, tabI, gmfU, gmfI, packed, w, scores = _ranking_case(native, gpu, rows, cols, tile)
    seen = K.exclusion(rows, cols, tile, gpu) if excl else None
    ref = native.topk_rows(scores, k, seen)
    got = native.neumf_topk(tabU, None, tabI, None, gmfU, gmfI, packed, w, k, seen)
    F.assert_same_bits(got[0], ref[0], "scores")
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    oracle = K.Ranking(scores, seen).topk(k)
    assert torch.equal(got[1], oracle[1]) and torch.equal(got[2], oracle[2])
    native.check_oob(gpu)


@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("tile,claim,mt", [(32, 32, 1), (32, 512, 3), (1024, 1024, 1), (1024, 1024, 3), (8192, 8192, 1), (8192, 8192, 3)])
def test_rank_is_score_then_rank(native, gpu, tile, claim, mt, excl):
    """claim: the range the plan picks (three users with several targets stay at the rank sink's 512-column floor)."""
    rows, cols = _shape(tile)
    assert native.ranking_plan("mlp_rank", rows, cols, mt)[:2] == (claim, -(-cols // claim))
    tabU, tabI, gmfU, gmfI, packed, w, scores = _ranking_case(native, gpu, rows, cols, tile)
    seen = K.exclusion(rows, cols, tile, gpu) if excl else None
    tg = K.targets(rows, cols, mt, gpu)
    ref = native.rank_rows(scores, tg, seen)
    got = native.neumf_rank(tabU, None, tabI, None, gmfU, gmfI, packed, w, tg, mt, seen)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    oracle = K.Ranking(scores, seen).rank(tg)
    assert torch.equal(got[0], oracle[0]) and torch.equal(got[1], oracle[1])
    native.check_rank_overflow(gpu)
    native.check_oob(gpu)


def test_topk_through_an_item_list_and_user_ids(native, gpu):
    """Listed users (repeats allowed) against a permuted item list: the ids reach both of a side's tables."""
    rows, cols = _shape(32)
    tabU, tabI, gmfU, gmfI, packed, w, _ = _ranking_case(native, gpu, rows, cols, 32)
    users = torch.tensor([2, 0, 2, 1, 1], device=gpu)
    items = torch.randperm(cols, generator=torch.Generator().manual_seed(4))[:77].to(gpu)
    scores = native.neumf_score(tabU, users.repeat_interleave(77), tabI, items.repeat(5), gmfU, gmfI, packed, w).view(5, 77)
    ref, got = native.topk_rows(scores, 10), native.neumf_topk(tabU, users, tabI, items, gmfU, gmfI, packed, w, 10)
    F.assert_same_bits(got[0], ref[0], "scores")
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])


@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("tower,D", [((128, 128, 64), 64), ((128, 128, 64), 128), ((64, 128, 0), 40), ((128, 256, 128), 128)])
def test_wide_gmf_rows_in_the_full_catalogue_waves(native, gpu, tower, D, excl):
    """D above 32 on the towers whose waves request four chunks of a column's GMF row ahead and load the others after the last sum
    (both halves of gmf_dot_t in one row), up to the full 512-byte t row in LDS; the 256-128 tower, which requests none, at that
    width too.  Random fp32 data; 157 columns: five ranges of 32, the last ragged."""
    tabs, ws, bs, w = _random_case(tower, D, 31 * D + tower[1])
    d = [t.to(gpu) for t in tabs]
    packed, w = native.PackedMLP([x.to(gpu) for x in ws], [x.to(gpu) for x in bs]), w.to(gpu)
    users = torch.arange(0, N_USERS, 9, device=gpu)
    rows, cols = users.numel(), N_ITEMS
    assert native.ranking_plan("mlp_topk", rows, cols, 10)[:2] == (32, 5) and native.ranking_plan("mlp_rank", rows, cols, 3)[0] == 512
    scores = native.neumf_score(d[0], users.repeat_interleave(cols), d[1], torch.arange(cols, device=gpu).repeat(rows), d[2], d[3],
                                packed, w).view(rows, cols)
    seen = K.exclusion(rows, cols, 64, gpu) if excl else None
    ref, got = native.topk_rows(scores, 10, seen), native.neumf_topk(d[0], users, d[1], None, d[2], d[3], packed, w, 10, seen)
    F.assert_same_bits(got[0], ref[0], "scores")
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    for mt in (1, 3):
        tg = K.targets(rows, cols, mt, gpu)
        ref, got = native.rank_rows(scores, tg, seen), native.neumf_rank(d[0], users, d[1], None, d[2], d[3], packed, w, tg, mt, seen)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), mt
    native.check_rank_overflow(gpu)
    native.check_oob(gpu)


def test_front_ends_take_a_neumf_on_every_route(native, gpu, monkeypatch):
    from deeprecommendation_amd import ranking_eval, recommend
    m = _neumf(gpu, 4).eval()
    users = torch.arange(0, N_USERS, 3, device=gpu)
    B = users.numel()
    seen = K.exclusion(B, N_ITEMS, 64, gpu)
    tg = K.targets(B, N_ITEMS, 2, gpu)
    calls = []
    for name in ("neumf_topk", "neumf_rank"):
        fn = getattr(native, name)
        monkeypatch.setattr(native, name, lambda *a, _fn=fn, _n=name, **kw: (calls.append(_n), _fn(*a, **kw))[1])
    a = recommend.top_k_items(m, users, 10, exclude=seen)
    b = recommend.top_k_items(m, users, 10, exclude=seen, fused=False)
    assert calls == ["neumf_topk"]
    F.assert_same_bits(a[0], b[0], "top_k_items")
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    ra = ranking_eval.rank_of_items(m, users, tg, exclude=seen)
    rb = ranking_eval.rank_of_items(m, users, tg, exclude=seen, fused=False)
    assert calls == ["neumf_topk", "neumf_rank"]
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    metrics = ranking_eval.eval_full_ranking(m, users, tg, exclude=seen, cutoffs=(10,))
    assert 0.0 <= metrics["hr@10"] <= 1.0 and calls == ["neumf_topk", "neumf_rank", "neumf_rank"]
    with pytest.raises(ValueError, match="needs a dot-product readout; NeuMF"):
        recommend.top_k_items(m, users, 10, fused=True)
    with pytest.raises(ValueError, match="graph= is only taken by a GraphNCF, not by NeuMF"):
        recommend.top_k_items(m, users, 10, graph=object())
    with pytest.raises(ValueError, match="profiles= is only taken by an AttentionNCF, not by NeuMF"):
        ranking_eval.rank_of_items(m, users, tg, profiles=(None, None))
    small = _neumf(gpu, 5, mf_dim=12).eval()          # no kernel: score-then-select through the torch-ops forward
    s = recommend.top_k_items(small, users, 5)
    assert s[0].shape == (B, 5) and len(calls) == 3


# ------------------------------------------------------------------------------------------------------------------ training
def test_one_step_gradients_through_the_hip_blocks(native, gpu):
    """Every parameter's gradient of one BCE step through the HIP autograd blocks against float64 autograd of the same model, beside
    the fp32 torch-ops path (train_with_torch_ops) against the same float64 gradients.  Both fp32 paths evaluate one function in
    different summation orders, so the HIP error may be at most 4 x the torch-ops error (slack for order, not for a bug).  Error of a
    parameter: max |g - g64| over its entries.  Eleven of the twelve parameters are held to exactly that.  The twelfth, predict.bias, has ONE
    entry: its torch-ops error is the rounding of a single sum, which is 0 whenever that sum happens to round to float64's value, and
    4 x 0 would demand float64's bits of the HIP column sum.  For that parameter alone the torch-ops error is taken as at least half an
    fp32 ulp of the entry, the error an fp32 result cannot be held below; the raw ratio is printed beside it."""
    m = _neumf(gpu, 6, mf_dim=8, item_emb=40, user_emb=24, mlp_dense_layers=[128]).train()
    g = torch.Generator().manual_seed(8)
    B = 257
    users, items = torch.randint(0, N_USERS, (B,), generator=g).to(gpu), torch.randint(0, N_ITEMS, (B,), generator=g).to(gpu)
    labels = torch.randint(0, 2, (B, 1), generator=g).to(gpu)

    def grads(model, dtype):
        model.zero_grad()
        out = model(users, items)
        assert out.dtype == dtype and out.shape == (B, 1)
        torch.nn.functional.binary_cross_entropy_with_logits(out, labels.to(dtype), reduction="sum").backward()
        return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}

    m64 = copy.deepcopy(m).double()
    m64.train_with_torch_ops = True
    m32 = copy.deepcopy(m)
    m32.train_with_torch_ops = True
    g64, g32, ghip = grads(m64, torch.float64), grads(m32, torch.float32), grads(m, torch.float32)
    assert set(ghip) == set(g64) and len(g64) == 12
    worst = {}
    for name, ref in g64.items():
        assert float(ref.abs().max()) > 0, name
        e_hip, raw_32 = float((ghip[name] - ref).abs().max()), float((g32[name] - ref).abs().max())
        e_32 = raw_32
        if ref.numel() == 1:                          # predict.bias: see the docstring
            e_32 = max(raw_32, float(np.spacing(np.float32(ref.abs().max()))) / 2)
        worst[name] = e_hip / e_32 if e_32 else (0.0 if e_hip == 0.0 else float("inf"))
        print(f"{name}: hip {e_hip:.3e} torch-ops {raw_32:.3e} (bound taken against {e_32:.3e}) ratio {worst[name]:.2f}")
    assert max(worst.values()) <= 4.0, worst


@pytest.mark.parametrize("loss", ["bce", "bpr"])
def test_fit_implicit_trains_a_neumf(native, gpu, loss):
    from deeprecommendation_amd import implicit
    from deeprecommendation_amd.neural_collaborative_filtering.models.neumf import NeuMF
    rng = np.random.default_rng(12)
    u = np.repeat(np.arange(64), 10)
    i = (u * 7 + rng.integers(0, 12, size=u.size)) % 48          # each user's items sit in a band of the catalogue
    tu, ti, hu, hi = implicit.leave_one_out(u, i, seed=1)
    data = implicit.ImplicitFeedback(tu, ti, 64, 48, device=gpu)
    torch.manual_seed(13)
    m = NeuMF(item_dim=48, user_dim=64, mf_dim=8, item_emb=40, user_emb=24, mlp_dense_layers=[128]).to(gpu)
    hist = implicit.fit_implicit(m, data, negatives=4, loss=loss, epochs=2, batch_size=64, lr=0.01, seed=2)["train_loss"]
    assert len(hist) == 2 and hist[1] < hist[0], hist
    users, held = torch.from_numpy(hu).to(gpu), torch.from_numpy(hi).to(gpu)
    cand = implicit.sampled_candidates(data, users, held, n_candidates=9, seed=3)
    metrics = implicit.eval_sampled(m, users, held, cand, cutoffs=(5,))
    rank, ranked = implicit.rank_sampled(m, users, held, cand)
    assert 0.0 <= metrics["hr@5"] <= 1.0 and int(ranked.min()) == 10 and rank.numel() == users.numel()
